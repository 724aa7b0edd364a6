"""The float64 model of the phase-lag family (plv, pli, wpli, wpli_debiased) from single-trial
cross spectra and from tapered spectra, written from the definitions, and the per-element error bound of a float32
accumulation, computed from the model alone.  Shared by tests/test_phaselag.py (CPU emulation) and
tests/test_gpu_phaselag.py.

Definitions.  S_t = sum_k x_ik conj(x_jk), s_t = Im S_t; over the T trials A = sum s_t, B = sum |s_t|, Q = sum s_t^2,
N = sum sign(s_t) (sign(0) = 0), U = sum of the unit phasors of S_t (1 for S_t = 0):
    plv = |U| / T,  pli = |N| / T,  wpli = |A| / B (0 where B = 0),  wpli_debiased = (A^2 - Q) / (B^2 - Q) (0 where <= 0);
the diagonal of the last three is exactly 0.

Bound, with u = 2^-24 and gamma_n = n u / (1 - n u).  A float32 chain of 2K fused multiply-adds leaves
|ds_t| <= delta_t = gamma_(2K+2) M_t, M_t = sum_k (|Im x_ik| |Re x_jk| + |Re x_ik| |Im x_jk|); T float32 additions carry it to
    E = (1 + gamma_T) sum delta_t,   dA = dB = E + gamma_T (B + E),
    dQ = gamma_T Q + 2 (1 + gamma_T) sum |s_t| delta_t + sum delta_t^2,
    wpli:           tol = 2 (2 dA / (B - dA) + 2u)
    wpli_debiased:  tol = 2 ((dnum + |result| dden) / (den - dden) + 2u),  dnum = 2 |A| dA + dA^2 + dQ,  dden = 2 B dA + dA^2 + dQ
(the leading 2: the second-order terms of a first-order bound).  pli: N is an exact integer unless a trial is FRAGILE,
|s_t| <= 4 delta_t; elsewhere the result agrees within 2u, a fragile element may differ by 2 (its fragile trials) / T.
plv: K7's own criterion (tests/test_gpu_pair_kernels.py: rtol 1e-4, atol_rel 2e-5).

Conditions on the INPUTS, asserted on the model before anything is compared (check): at most 0.1 % of the off-diagonal
elements fragile; elements whose wpli / wpli_debiased bound exceeds 1e-3 are left out of that comparison, at most 1 %."""
import numpy as np

from parity import assert_parity

U32 = 2.0 ** -24
MEASURES = ("plv", "pli", "wpli", "wpli_debiased")
MEASURE_CODE = {"pli": 0, "wpli": 1, "wpli_debiased": 2}        # SPYHIP_PHASELAG_*
BOUND_CAP, ILL_SHARE, FRAGILE_SHARE = 1e-3, 0.01, 0.001

# (C, F, T, K) of the kernel cases
SHAPES = [(70, 5, 8, 3),        # three tile rows, a 6-channel partial tile
          (33, 3, 2, 1),        # one channel into the second tile, one taper, the shortest double-buffer sequence
          (64, 2, 5, 17),       # exact tiles; 17 tapers take the generic staging walk
          (31, 4, 3, 7),        # a single partial tile
          (32, 9, 3, 2)]        # F = 9: frequency slots that return early under the XCD mapping


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def spectra(C, F, T, K, seed=None):
    """(T, K, F, C) complex64: complex Gaussian spectra + 0.8 x a common source per (trial, taper, frequency) seen through
    a random phase per channel; the last channel all zero"""
    rng = np.random.default_rng(1000 * C + 10 * F + T + K if seed is None else seed)
    x = rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))
    src = rng.normal(size=(T, K, F, 1)) + 1j * rng.normal(size=(T, K, F, 1))
    x = x + 0.8 * src * np.exp(1j * rng.uniform(-np.pi, np.pi, size=C))
    x[..., C - 1] = 0
    return x.astype(np.complex64)


def cross_spectra(spec):
    """(T, K, F, C) -> S (T, F, C, C) complex128 and M (T, F, C, C) float64"""
    x = np.asarray(spec).astype(np.complex128)
    S = np.einsum("tkfi,tkfj->tfij", x, x.conj())
    re, im = np.abs(x.real), np.abs(x.imag)
    M = np.einsum("tkfi,tkfj->tfij", im, re) + np.einsum("tkfi,tkfj->tfij", re, im)
    return S, M


def sums(S):
    """A, B, Q, N, U over the trials (axis 0) of single-trial cross spectra"""
    S = np.asarray(S).astype(np.complex128)
    s = S.imag
    mod = np.abs(S)
    u = np.where(mod > 0, S / np.where(mod > 0, mod, 1.0), 1.0)
    return s.sum(0), np.abs(s).sum(0), (s * s).sum(0), np.sign(s).sum(0), u.sum(0)


def measures(S, diagonal=True):
    """the four results (float64) of single-trial cross spectra S (T, ..., Ci, Cj).  diagonal: Ci = Cj are the same channels
    and i = j is exactly 0 in pli, wpli and wpli_debiased"""
    T = np.asarray(S).shape[0]
    A, B, Q, N, U = sums(S)
    den = B * B - Q
    pos = den > 0
    out = {"plv": np.abs(U) / T, "pli": np.abs(N) / T,
           "wpli": np.where(B > 0, np.abs(A) / np.where(B > 0, B, 1.0), 0.0),
           "wpli_debiased": np.where(pos, (A * A - Q) / np.where(pos, den, 1.0), 0.0)}
    if diagonal:
        i = np.arange(out["pli"].shape[-1])
        for m in ("pli", "wpli", "wpli_debiased"):
            out[m][..., i, i] = 0.0
    return out


def from_spectra(spec, diagonal=True):
    return measures(cross_spectra(spec)[0], diagonal)


def bounds(S, M=None, K=1):
    """per element: tol of pli, wpli, wpli_debiased (inf where the bound's own denominator is not positive) and the
    number of fragile trials.  M = None: the s_t are inputs (single-trial cross spectra), delta_t = 0"""
    S = np.asarray(S).astype(np.complex128)
    T = S.shape[0]
    s = S.imag
    delta = np.zeros_like(s) if M is None else gamma(2 * K + 2) * M
    A, B, Q, _, _ = sums(S)
    gT = gamma(T)
    E = (1 + gT) * delta.sum(0)
    dA = E + gT * (B + E)
    dQ = gT * Q + 2 * (1 + gT) * (np.abs(s) * delta).sum(0) + (delta * delta).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_w = np.where(B - dA > 0, 2 * (2 * dA / (B - dA) + 2 * U32), np.inf)
        den = B * B - Q
        res = np.where(den > 0, (A * A - Q) / np.where(den > 0, den, 1.0), 0.0)
        dnum = 2 * np.abs(A) * dA + dA * dA + dQ
        dden = 2 * B * dA + dA * dA + dQ
        tol_d = np.where(den - dden > 0, 2 * ((dnum + np.abs(res) * dden) / (den - dden) + 2 * U32), np.inf)
    # where s_t = 0 in the model AND nothing is rounded (delta_t = 0) the kernel's sign is the model's: not fragile
    fragile = ((np.abs(s) <= 4 * delta) & (delta > 0)).sum(0)
    tol_p = 2 * U32 + 2.0 * fragile / T
    return {"pli": tol_p, "wpli": tol_w, "wpli_debiased": tol_d, "fragile": fragile}


def offdiag(shape, square=True):
    """mask of the elements that are compared under a bound: everything of a rectangle, the off-diagonal of a square"""
    m = np.ones(shape, dtype=bool)
    if square:
        i = np.arange(shape[-1])
        m[..., i, i] = False
    return m


def check(got, S, M=None, K=1, square=True, which=MEASURES, what="", mirrored=True):
    """got: {measure: float32 array}; every measure of `which` against the model of S under the bounds.  On a square the
    diagonal of pli / wpli / wpli_debiased must be exactly 0 and, where the finalizer mirrored the lower triangle
    (`mirrored`), every result exactly symmetric; results taken element by element from single-trial cross spectra are as
    symmetric as those are.  Returns the largest err/tol per measure."""
    want = measures(S, diagonal=square)
    b = bounds(S, M, K)
    off = offdiag(want["pli"].shape, square)
    # dead pairs (B = 0 in the model, e.g. the all-zero channel): exact zeros, compared as such
    dead = sums(S)[1] == 0
    n_off = int(off.sum())
    assert int(((b["fragile"] > 0) & off).sum()) <= FRAGILE_SHARE * n_off, (what, "too many fragile elements")
    worst = {}
    for m in which:
        g = np.asarray(got[m])
        assert g.dtype == np.float32 and g.shape == want[m].shape, (what, m, g.dtype, g.shape)
        assert np.isfinite(g).all(), (what, m, "non-finite")
        if square and mirrored:
            assert np.array_equal(g, np.swapaxes(g, -1, -2)), (what, m, "not symmetric")
        if m == "plv":
            assert_parity(g, want[m], rtol=1e-4, atol_rel=2e-5, what=f"{what} plv")
            continue
        if square:
            i = np.arange(g.shape[-1])
            assert np.all(g[..., i, i] == 0), (what, m, "diagonal not exactly 0")
        assert np.all(g[dead & off] == 0), (what, m, "dead pair not exactly 0")
        tol = b[m]
        keep = off & ~dead
        if m != "pli":
            ill = keep & ~(tol <= BOUND_CAP)
            assert int(ill.sum()) <= ILL_SHARE * n_off, (what, m, "too many ill-conditioned elements", int(ill.sum()))
            keep &= ~ill
        err = np.abs(g.astype(np.float64) - want[m])
        ratio = err[keep] / tol[keep]
        worst[m] = float(ratio.max()) if ratio.size else 0.0
        print(f"{what} {m}: max err/tol {worst[m]:.3f}, largest bound {float(tol[keep].max()) if ratio.size else 0:.2e}, "
              f"{int(keep.sum())} of {n_off} elements")
        assert worst[m] <= 1.0, (what, m, worst[m])
    return worst
