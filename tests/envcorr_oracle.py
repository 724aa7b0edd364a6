"""The float64 model of the envelope correlations (amplcorr, powcorr, powcorr_ortho) from tapered
spectra, written from the definitions, and the per-element error bound of the kernels' arithmetic, computed from the model
alone.  Shared by tests/test_envcorr.py (CPU emulation) and tests/test_gpu_envcorr.py.

Definitions.  Over the R = T K repetitions r = (trial, taper) of the complex64 spectra x_i(r) of one frequency - every
taper is a repetition - and with
    corr(X; E1a, E2a, E1b, E2b) = (X - E1a E1b / R) / sqrt(va vb),  va = E2a - E1a^2 / R,  vb = E2b - E1b^2 / R,
    0 where a variance is zero: v <= 2^-40 E2,
amplcorr (e = |x|) and powcorr (e = |x|^2) are corr(sum e_i e_j; sum e_i, sum e_i^2, sum e_j, sum e_j^2) with the diagonal
exactly 1 (0 for a channel without variance); powcorr_ortho has p = |x|^2, s = Im(x_i conj(x_j)), q_j|i = s^2 / p_i (0 where
p_i = 0), Z = sum s^2 = sum p_i q_j|i, c_j|i = corr(Z; sum p_i, sum p_i^2, sum q_j|i, sum q_j|i^2) and the result
(c_j|i + c_i|j) / 2 where both exist, else 0, with the diagonal exactly 0.  Everything is clamped to [-1, 1].

Bound, with u = 2^-24 and gamma_n = n u / (1 - n u).  The kernels hold |x|, p, 1 / p, s, s^2 and q in float32, form every
product of two of them in float64 (exact) and sum in float64, so only the float32 roundings count, and they do not grow
with R.  Roundings counted from csrc/envcorr_kernel.h:
    p = fma(re, re, im im): 2 (gamma_2);  |x| = sqrt(p): 3 (gamma_3);  1 / p: one division more, 3;
    s = fma(-re_i, im_j, im_i re_j): 2, bounded as the absolute error delta = gamma_3 (|Im x_i Re x_j| + |Re x_i Im x_j|);
    s^2 = s s: 1 more;  q = s^2 (1 / p): the rounding of s^2 aside, 3 + 1 = 4 (gamma_4).
amplcorr, powcorr (g = gamma_3, gamma_2; g2 = 2 g + g^2): dX = g2 X, dE1 = g E1, dE2 = g2 E2.  powcorr_ortho, per
repetition: d(s^2) = 2 |s| delta + delta^2 + gamma_1 (|s| + delta)^2, dq = ((1 + gamma_4) d(s^2) + gamma_4 s^2) / p,
d(q^2) = 2 q dq + dq^2; their sums are dZ, dG1 and dG2; dP1 = gamma_2 P1, dP2 = (2 gamma_2 + gamma_2^2) P2.  Then
    dcov = dX + (dE1a E1b + E1a dE1b + dE1a dE1b) / R,   dv = dE2 + (2 E1 dE1 + dE1^2) / R,
    first-order error of a correlation r:  dcov / sqrt(va vb) + |r| / 2 (dva / va + dvb / vb),
    tol = 2 (that + 2u)   (powcorr_ortho: the mean of the two directions' errors),   inf where v - dv <= 0.

Conditions on the INPUTS, asserted on the model before anything is compared (check): elements with tol > 1e-3 are left out,
at most 1 % of the off-diagonal elements; no variance has v / E2 between 2^-44 and 2^-36 (the zero-variance rule is then
decided alike by the model and by the kernels)."""
import numpy as np

U32 = 2.0 ** -24
MEASURES = ("amplcorr", "powcorr", "powcorr_ortho")
MEASURE_CODE = {"amplcorr": 0, "powcorr": 1, "powcorr_ortho": 2}        # SPYHIP_ENVCORR_*
PLANES = {"amplcorr": 1, "powcorr": 1, "powcorr_ortho": 5}
BOUND_CAP, ILL_SHARE = 1e-3, 0.01
ZERO_VAR = 2.0 ** -40
NEAR_ZERO_VAR = (2.0 ** -44, 2.0 ** -36)

# (C, F, T, K) of the kernel cases: K10's five, the second with four trials (two repetitions make every correlation +-1)
SHAPES = [(70, 5, 8, 3),        # three tile rows, a 6-channel partial tile
          (33, 3, 4, 1),        # one channel into the second tile, one taper
          (64, 2, 5, 17),       # exact tiles; 17 tapers take the generic staging walk
          (31, 4, 3, 7),        # a single partial tile
          (32, 9, 3, 2)]        # F = 9: frequency slots that return early under the XCD mapping


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def spectra(C, F, T, K, seed=None):
    """(T, K, F, C) complex64: complex Gaussian spectra + 0.8 x a common source per (trial, taper, frequency) seen through
    a random phase per channel, times a common log-normal gain exp(0.5 n) per (trial, taper, frequency); the last channel
    all zero, the last but one the constant 0.75 - 0.5j"""
    rng = np.random.default_rng(1000 * C + 10 * F + T + K if seed is None else seed)
    x = rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))
    src = rng.normal(size=(T, K, F, 1)) + 1j * rng.normal(size=(T, K, F, 1))
    x = x + 0.8 * src * np.exp(1j * rng.uniform(-np.pi, np.pi, size=C))
    x = x * np.exp(0.5 * rng.normal(size=(T, K, F, 1)))
    x[..., C - 1] = 0
    x[..., C - 2] = 0.75 - 0.5j
    return x.astype(np.complex64)


def _variance(E1, E2, R):
    """v and whether it counts as non-zero"""
    v = E2 - E1 * E1 / R
    return v, v > ZERO_VAR * E2


def _corr(X, E1a, E2a, E1b, E2b, R, dX=None, dE1a=None, dE2a=None, dE1b=None, dE2b=None):
    """the correlation (0 where a variance is zero), whether it exists, its first-order error (inf where v - dv <= 0; None
    without the d's) and the two v / E2"""
    va, oka = _variance(E1a, E2a, R)
    vb, okb = _variance(E1b, E2b, R)
    ok = oka & okb
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ok, (X - E1a * E1b / R) / np.sqrt(np.where(ok, va * vb, 1.0)), 0.0)
        rel = (np.where(E2a > 0, va / np.where(E2a > 0, E2a, 1.0), 0.0), np.where(E2b > 0, vb / np.where(E2b > 0, E2b, 1.0), 0.0))
        if dX is None:
            return r, ok, None, rel
        dcov = dX + (dE1a * E1b + E1a * dE1b + dE1a * dE1b) / R
        dva = dE2a + (2 * E1a * dE1a + dE1a * dE1a) / R
        dvb = dE2b + (2 * E1b * dE1b + dE1b * dE1b) / R
        good = ok & (va - dva > 0) & (vb - dvb > 0)
        sva, svb = np.where(good, va, 1.0), np.where(good, vb, 1.0)
        err = np.where(good, dcov / np.sqrt(sva * svb) + np.abs(r) / 2 * (dva / sva + dvb / svb), np.inf)
    return r, ok, err, rel


def model(spec, measure):
    """spec (T, K, F, C) complex64 -> dict: `want` (F, C, C) float64, `tol` (F, C, C), `defined` (F, C, C) bool (False: a
    variance is zero, the result is exactly 0 off the diagonal) and `rel` (F, n), every v / E2 that decides one"""
    x = np.asarray(spec)
    assert x.dtype == np.complex64 and x.ndim == 4
    T, K, F, C = x.shape
    R = T * K
    x = x.reshape(R, F, C).astype(np.complex128)
    re, im = x.real, x.imag
    p = re * re + im * im
    diag = np.arange(C)
    if measure in ("amplcorr", "powcorr"):
        e, g = (np.sqrt(p), gamma(3)) if measure == "amplcorr" else (p, gamma(2))
        g2 = 2 * g + g * g
        X = np.einsum("rfi,rfj->fij", e, e)
        E1, E2 = e.sum(0), (e * e).sum(0)
        a = (E1[:, :, None], E2[:, :, None])
        b = (E1[:, None, :], E2[:, None, :])
        r, ok, err, rel = _corr(X, *a, *b, R, g2 * X, g * a[0], g2 * a[1], g * b[0], g2 * b[1])
        r = np.clip(r, -1.0, 1.0)
        r[:, diag, diag] = ok[:, diag, diag]
        return {"want": r, "tol": 2 * (err + 2 * U32), "defined": ok, "rel": np.concatenate([v.reshape(F, -1) for v in rel], axis=1)}
    assert measure == "powcorr_ortho"
    # [r, f, i, j]: s = Im(x_i conj(x_j)), q = q_j|i = s^2 / p_i; the other direction is the transpose
    s = im[:, :, :, None] * re[:, :, None, :] - re[:, :, :, None] * im[:, :, None, :]
    delta = gamma(3) * (np.abs(im[:, :, :, None] * re[:, :, None, :]) + np.abs(re[:, :, :, None] * im[:, :, None, :]))
    s2 = s * s
    ds2 = 2 * np.abs(s) * delta + delta * delta + gamma(1) * (np.abs(s) + delta) ** 2
    pi = p[:, :, :, None]
    inv = np.where(pi > 0, 1.0 / np.where(pi > 0, pi, 1.0), 0.0)
    q = s2 * inv
    dq = ((1 + gamma(4)) * ds2 + gamma(4) * s2) * inv
    Z, dZ = s2.sum(0), ds2.sum(0)
    G1, dG1 = q.sum(0), dq.sum(0)
    G2, dG2 = (q * q).sum(0), (2 * q * dq + dq * dq).sum(0)
    g = gamma(2)
    g2 = 2 * g + g * g
    P1, P2 = p.sum(0)[:, :, None], (p * p).sum(0)[:, :, None]
    c, ok, err, rel = _corr(Z, P1, P2, G1, G2, R, dZ, g * P1, g2 * P2, dG1, dG2)          # c_j|i at [f, i, j]
    both = ok & ok.transpose(0, 2, 1)
    r = np.where(both, 0.5 * (c + c.transpose(0, 2, 1)), 0.0)
    r = np.clip(r, -1.0, 1.0)
    r[:, diag, diag] = 0.0
    both[:, diag, diag] = False
    off = ~np.eye(C, dtype=bool)
    return {"want": r, "tol": 2 * (0.5 * (err + err.transpose(0, 2, 1)) + 2 * U32), "defined": both,
            "rel": np.concatenate([rel[0][:, :, 0], rel[1][:, off]], axis=1)}


def measures(spec):
    return {m: model(spec, m)["want"] for m in MEASURES}


def check(got, spec, which=MEASURES, what="", real_bins=(), models=None):
    """got: {measure: (F, C, C) float32}; every measure of `which` against the model of spec (T, K, F, C) under its bound:
    finite, inside [-1, 1], exactly symmetric, the exact diagonal, exact zeros where a variance is zero, and err <= tol
    elsewhere.  `real_bins`: frequencies whose spectra are real (0 Hz, Nyquist) - s is a rounding residue there, which no
    bound covers - are held to everything but the bound.  `models`: {measure: model(spec, measure)} computed already.
    Returns the largest err / tol per measure."""
    worst = {}
    for m in which:
        mod = models[m] if models is not None else model(spec, m)
        want, tol, defined = mod["want"], mod["tol"], mod["defined"]
        F, C, _ = want.shape
        bound = np.ones((F, 1, 1), dtype=bool)
        bound[list(real_bins)] = False
        lo, hi = NEAR_ZERO_VAR
        rel = mod["rel"][bound[:, 0, 0]]
        assert not np.any((rel > lo) & (rel < hi)), (what, m, "a variance near the zero-variance threshold")
        g = np.asarray(got[m])
        assert g.dtype == np.float32 and g.shape == want.shape, (what, m, g.dtype, g.shape)
        assert np.isfinite(g).all() and np.all(np.abs(g) <= 1), (what, m, "not finite or outside [-1, 1]")
        assert np.array_equal(g, g.transpose(0, 2, 1)), (what, m, "not symmetric")
        i = np.arange(C)
        assert np.array_equal(g[:, i, i], want[:, i, i].astype(np.float32)), (what, m, "diagonal")
        assert set(np.unique(g[:, i, i])) <= {0.0, 1.0} if m != "powcorr_ortho" else not g[:, i, i].any(), (what, m, "diagonal")
        off = ~np.eye(C, dtype=bool)[None] & bound
        n_off = int(off.sum())
        assert np.all(g[off & ~defined] == 0), (what, m, "a pair with a channel without variance is not exactly 0")
        keep = off & defined
        ill = keep & ~(tol <= BOUND_CAP)
        assert int(ill.sum()) <= ILL_SHARE * n_off, (what, m, "too many ill-conditioned elements", int(ill.sum()))
        keep &= ~ill
        err = np.abs(g.astype(np.float64) - want)
        ratio = err[keep] / tol[keep]
        worst[m] = float(ratio.max()) if ratio.size else 0.0
        print(f"{what} {m}: max err/tol {worst[m]:.3f}, largest bound {float(tol[keep].max()) if ratio.size else 0:.2e}, "
              f"mean |r| {float(np.abs(want[keep]).mean()) if ratio.size else 0:.2f}, {int(keep.sum())} of {n_off} elements "
              f"({int(ill.sum())} left out)")
        assert worst[m] <= 1.0, (what, m, worst[m])
    return worst
