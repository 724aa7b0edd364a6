"""Float64 model of the phase slope index (K13: syncopy_amd/csrc/phaseslope_kernel.h), TEST INFRASTRUCTURE ONLY: the
definition of include/spyhip.h applied to a given complex64 coherency, its jackknife, the error bound that follows from
the definition alone, and the inputs of the kernel shapes."""
import numpy as np

# (channels, frequencies, half width): degenerate, tile edges, exactly one valid bin, one edge, off-diagonal full tiles;
# 41 frequencies of 33 channels are 3, 2 and 2 frequency runs of the kernel for h = 1, 5 and 0 (runs of 16 output bins, of
# 32 edges for h = 0): bin 20 of h = 5 sums the edges 15 ... 24 across the run boundary at bin 21
SHAPES = ((1, 5, 1), (31, 9, 1), (32, 9, 1), (33, 9, 1), (33, 17, 8), (33, 2, 0), (64, 40, 3), (33, 41, 1), (33, 41, 5),
          (33, 41, 0))
RUNS = {(64, 40, 3): 3, (33, 41, 1): 3, (33, 41, 5): 2, (33, 41, 0): 2}      # every other shape is one run
SCALE = 0.25                       # of the raw accumulator: a power of two, so that csd = raw * SCALE exactly


def spectra(Cn, F, seed=0, nrep=6):
    """(nrep, F, C) complex128: white spectra plus a common component that arrives c % 4 bins of phase later in channel c;
    the last channel is all zero"""
    rng = np.random.default_rng(1000 * Cn + F + seed)
    x = rng.normal(size=(nrep, F, Cn)) + 1j * rng.normal(size=(nrep, F, Cn))
    s = rng.normal(size=(nrep, F, 1)) + 1j * rng.normal(size=(nrep, F, 1))
    f = np.arange(F)[None, :, None]
    x = x + 1.5 * s * np.exp(-2j * np.pi * f * (np.arange(Cn) % 4)[None, None, :] / max(2 * F, 8))
    x[..., -1] = 0
    return x


def hermitian_csd(x):
    """(F, C, C) complex64, exactly Hermitian with a real diagonal: S_ij = <x_i conj(x_j)> over the repetitions"""
    S = np.einsum("rfi,rfj->fij", x, np.conj(x)) / x.shape[0]
    lo = np.tril(S).astype(np.complex64)
    i = np.arange(S.shape[1])
    lo[:, i, i] = lo[:, i, i].real
    return lo + np.conj(np.tril(lo, -1)).transpose(0, 2, 1)


def raw_accumulator(csd):
    """the unscaled lower triangle as spyhip_csd_accumulate leaves it: whole tiles on and below the diagonal, a rounding
    residue as the diagonal's imaginary part, and NaN in the strictly upper tiles, which nobody may read"""
    raw = (csd / np.float32(SCALE)).astype(np.complex64)
    assert np.array_equal(raw * np.complex64(SCALE), csd)
    Cn = csd.shape[1]
    i = np.arange(Cn)
    raw[:, i, i] += np.complex64(1e-6j)
    t = i // 32
    raw[:, t[:, None] < t[None, :]] = np.nan
    return raw


def psi_model(coh, half):
    """psi of the complex64 coherency (F, C, C): float64 (F, C, C), whole planes NaN where the band does not fit; half = 0:
    (1, C, C).  Non-finite coherency counts as 0."""
    c = np.array(coh, dtype=np.complex64)
    F = c.shape[0]
    assert F >= 2 and 0 <= 2 * half <= F - 1
    c[~np.isfinite(c)] = 0
    x, y = c.real.astype(np.float64), c.imag.astype(np.float64)
    p = x[:-1] * y[1:] - y[:-1] * x[1:]                      # both products exact
    if half == 0:
        return p.sum(axis=0)[None]
    out = np.full(c.shape, np.nan)
    for k in range(half, F - half):
        out[k] = p[k - half:k + half].sum(axis=0)
    return out


def bound(model, F, half):
    """|got - m| <= 2^-24 |m| + (F + 2h) max(2h, F - 1 if h = 0) 2^-52: one rounding to float32, and float64 sums of at most
    F + 2h terms, in either order, whose partial sums stay below the number of edges of a band"""
    return 2.0 ** -24 * np.abs(model) + (F + 2 * half) * max(2 * half, F - 1 if half == 0 else 0) * 2.0 ** -52


def check(got, coh, half, what=""):
    """every assertion of one result (F or 1, C, C) float32 against the model on `coh`; returns the largest err / tol"""
    F, Cn = coh.shape[:2]
    m = psi_model(coh, half)
    assert got.shape == m.shape and got.dtype == np.float32, (what, got.shape, got.dtype)
    valid = np.zeros(m.shape[0], dtype=bool)
    valid[half:F - half if half else 1] = True
    assert np.isnan(got[~valid]).all() and np.isfinite(got[valid]).all(), what       # NaN planes, and nowhere else
    g, mv = got[valid], m[valid]
    tol = bound(mv, F, half)
    worst = float((np.abs(g - mv) / tol).max())
    print(f"{what}: err/tol {worst:.3g}")
    assert worst <= 1.0, (what, worst)
    assert np.array_equal(g, -g.transpose(0, 2, 1)), what                            # exact antisymmetry
    i = np.arange(Cn)
    assert not g[:, i, i].any() and not np.signbit(g[:, i, i]).any(), what           # the diagonal: +0
    return worst


def coherency64(S):
    """K5's coherency of a complex128 CSD (F, C, C), diagonal real, rounded to complex64"""
    d = np.real(np.einsum("fii->fi", S))
    with np.errstate(all="ignore"):
        c = S / np.sqrt(d[:, :, None] * d[:, None, :])
    i = np.arange(S.shape[1])
    c[:, i, i] = c[:, i, i].real
    return c.astype(np.complex64)


def jackknife_model(single, half):
    """kept single-trial CSDs (T, F, C, C) -> (direct, bias, var) as statistics/jackknifing.py: leave-one-out averages in
    float64, K5's coherency rounded to complex64, psi_model; bias = (T - 1)(mean_t r_t - direct), var = (T - 1) sum_t
    (mean r - r_t)^2"""
    S = np.asarray(single, dtype=np.complex128)
    T = S.shape[0]
    mean = S.mean(axis=0)
    direct = psi_model(coherency64(mean), half)
    rep = np.stack([psi_model(coherency64((T * mean - S[t]) / (T - 1)), half) for t in range(T)])
    avg = rep.mean(axis=0)
    return direct, (T - 1) * (avg - direct), (T - 1) * ((avg - rep) ** 2).sum(axis=0)
