"""Float64 model of K9 (jack_coh_kernel: streaming leave-one-out replicates of the coherence) with the element-wise
rounding bound of a float32 evaluation, the seeded inputs and the case tables shared by the emulator and the device
tests of the two pair kernels (K7 ppc_accum_kernel, K9).  Plain NumPy; nothing here reads the kernel.

The model is handed what the kernel is handed: spec (T, K, F, C) complex64, S (F, C, C) complex64, `direct` in the
requested output kind, the kind and T.  Per left-out trial t, in float64 / complex128:

    S_t = (1/K) sum_k x_i conj(x_j)        L = (T S - S_t) / (T - 1)        c = L_ij / sqrt(L_ii L_jj)
    d_t = conv(c) - direct                 sum_d = sum_t d_t                sum_d2 = sum_t |d_t|^2

Bound.  The kernel forms L in float32 the way the reference forms it in complex64: T*S and the subtraction round at
the size of T|S|, not of |L|.  With the base error u = 8 * 2^-24 (the 8 ulp at unit scale of
parity.jackknife_tolerances) and, per trial and pair, the conditioning of c on those roundings

    g = T/(T-1) * ( |S_ij| / sqrt(L_ii L_jj) + |c|/2 * (S_ii / L_ii + S_jj / L_jj) )

(first term: the rounding of T S_ij carried into the numerator; second: those of T S_ii, T S_jj carried through
1/sqrt(L_ii L_jj)), a replicate is good to e = u * max(1, g).  'pow' = |c|^2 turns that into 2|c|e + e^2, 'angle' into
e / |c|; the other kinds are 1-Lipschitz in c and keep e.  Then

    tol(sum_d) = sum_t e            tol(sum_d2) = sum_t (2 e |d_t| + e^2)

The complex kind compares the modulus of the complex difference.

Conditions on the inputs (asserted on the model alone, before anything is compared): max g <= 32, and for 'angle'
every |c| >= 0.3 and every |angle(c)| < 3 - no replicate near the branch cut."""
import functools

import numpy as np

KINDS = ("pow", "abs", "real", "imag", "angle", "absreal", "absimag", "complex")
U = 8.0 * 2.0 ** -24
G_CAP = 32.0

# K9: (C, F, T, K, kind, trials per launch).  K = 16 | 17: both sides of the staging switch (64 K <= | > 1024); F below
# 8, at 8 and 9, at 15 / 16 / 17: blocks that return early under fchunk = (F + 7) >> 3; one to five tile rows;
# launches of one trial; all eight kinds, the two whose mirrored store changes sign on shapes with off-diagonal tiles.
# (T = 2 with K = 2 has g = 224: T = 2 cases use K >= 4.)
JACK_CASES = [
    (1, 5, 4, 3, "abs", [4]),
    (31, 1, 7, 20, "absimag", [7]),
    (32, 16, 2, 33, "absreal", [1, 1]),
    (33, 3, 2, 4, "complex", [2]),
    (33, 9, 5, 17, "imag", [1, 4]),
    (33, 9, 5, 17, "angle", [5]),
    (63, 15, 3, 17, "imag", [3]),
    (64, 8, 4, 1, "real", [3, 1]),
    (65, 7, 4, 16, "complex", [2, 2]),
    (97, 17, 3, 2, "pow", [3]),
    (129, 2, 3, 2, "angle", [2, 1]),
    (33, 8, 40, 7, "pow", [40]),
]
# K7: the new shapes of test_ppc_kernel (the first launch holds one trial)
PPC_EDGE_CASES = [(33, 9, 6, 17), (65, 7, 5, 16), (31, 15, 5, 33), (97, 2, 5, 2)]


def case_id(case):
    return "-".join(str(v) if not isinstance(v, list) else "+".join(map(str, v)) for v in case)


# With one or two tapers and three or four trials a leave-one-out power can come out small by chance (max g of
# (64, 8, 4, 1) over six consecutive seeds: 152, 19, 65, 97, 18, 18).  Where the first seed of a shape misses the
# conditions on the inputs, the seed moves on by this much - judged on the float64 model alone, before any kernel ran.
SEED_STEP = {(64, 8, 4, 1): 5}


def case_seed(case):
    """One seed per shape: the two kinds tried at (33, 9, 5, 17) see the same spectra."""
    C, F, T, K = case[:4]
    return ((C * 100 + F) * 100 + T) * 100 + K + SEED_STEP.get((C, F, T, K), 0)


def convert(c, kind):
    """The output conversion of a coherency (csd.py:118-172 of the reference)."""
    if kind == "complex":
        return c
    if kind == "pow":
        return np.abs(c) ** 2
    if kind == "abs":
        return np.abs(c)
    if kind == "real":
        return c.real
    if kind == "imag":
        return c.imag
    if kind == "angle":
        return np.angle(c)
    if kind == "absreal":
        return np.abs(c.real)
    if kind == "absimag":
        return np.abs(c.imag)
    raise ValueError(kind)


def _single_trial_csd(x):
    """x (K, F, C) complex128 -> (F, C, C): (1/K) sum_k x_i conj(x_j)."""
    return np.einsum("kfi,kfj->fij", x, x.conj()) / x.shape[0]


def _coherency(L):
    p = np.einsum("fii->fi", L).real
    return L / np.sqrt(p[:, :, None] * p[:, None, :]), p


def make_inputs(seed, C, F, T, K, kind):
    """Seeded spectra with a strong common component (coherences around 0.85, phases within (-2, 2)) and the S and
    `direct` the kernel is handed: the float64 trial average rounded to complex64, its float64 coherency converted and
    rounded to float32 / complex64."""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))
    common = rng.normal(size=(T, K, F, 1)) + 1j * rng.normal(size=(T, K, F, 1))
    phi = rng.uniform(-1.0, 1.0, size=C)
    spec = (0.6 * N + 1.5 * common * np.exp(1j * phi)).astype(np.complex64)
    S = np.zeros((F, C, C), np.complex128)
    for t in range(T):
        S += _single_trial_csd(spec[t].astype(np.complex128))
    S = (S / T).astype(np.complex64)
    c, _ = _coherency(S.astype(np.complex128))
    direct = convert(c, kind).astype(np.complex64 if kind == "complex" else np.float32)
    return spec, S, direct


def model(spec, S, direct, kind, T):
    """Float64 sums of d_t and |d_t|^2 over the trials of spec, their element-wise tolerances and the figures the
    conditions on the inputs are stated in: dict(sum_d, sum_d2, tol_d, tol_d2, g_max, c_min, angle_max)."""
    assert spec.dtype == np.complex64 and S.dtype == np.complex64 and spec.shape[0] == T
    assert direct.dtype == (np.complex64 if kind == "complex" else np.float32)
    _, K, F, C = spec.shape
    S = S.astype(np.complex128)
    Sp = np.einsum("fii->fi", S).real
    direct = direct.astype(np.complex128 if kind == "complex" else np.float64)
    sum_d = np.zeros((F, C, C), direct.dtype)
    sum_d2 = np.zeros((F, C, C), np.float64)
    tol_d, tol_d2 = np.zeros((F, C, C)), np.zeros((F, C, C))
    g_max, c_min, angle_max = 0.0, np.inf, 0.0
    for t in range(T):
        L = (T * S - _single_trial_csd(spec[t].astype(np.complex128))) / (T - 1)
        c, Lp = _coherency(L)
        assert (Lp > 0).all()
        ac = np.abs(c)
        r = Sp / Lp
        g = T / (T - 1) * (np.abs(S) / np.sqrt(Lp[:, :, None] * Lp[:, None, :])
                           + 0.5 * ac * (r[:, :, None] + r[:, None, :]))
        e = U * np.maximum(1.0, g)
        if kind == "pow":
            e = 2.0 * ac * e + e * e
        elif kind == "angle":
            e = e / ac
        d = convert(c, kind) - direct
        sum_d += d
        sum_d2 += np.abs(d) ** 2
        tol_d += e
        tol_d2 += 2.0 * e * np.abs(d) + e * e
        g_max = max(g_max, float(g.max()))
        c_min = min(c_min, float(ac.min()))
        angle_max = max(angle_max, float(np.abs(np.angle(c)).max()))
    return dict(sum_d=sum_d, sum_d2=sum_d2, tol_d=tol_d, tol_d2=tol_d2, g_max=g_max, c_min=c_min, angle_max=angle_max)


@functools.lru_cache(maxsize=None)
def _case_data(C, F, T, K, kind, seed):
    spec, S, direct = make_inputs(seed, C, F, T, K, kind)
    m = model(spec, S, direct, kind, T)
    assert_conditions(m, kind)
    for a in (spec, S, direct, *[v for v in m.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return spec, S, direct, m


def case_data(case):
    """(spec, S, direct, model) of a case, computed once and shared read-only; the conditions on the inputs hold."""
    C, F, T, K, kind = case[:5]
    return _case_data(C, F, T, K, kind, case_seed(case))


def assert_conditions(m, kind):
    """The conditions on the inputs; no tolerance of the comparison."""
    assert m["g_max"] <= G_CAP, m["g_max"]
    if kind == "angle":
        assert m["c_min"] >= 0.3 and m["angle_max"] < 3.0, (m["c_min"], m["angle_max"])


def err_over_tol(sum_d, sum_d2, m):
    """(max err/tol of sum_d, of sum_d2) against the model; the complex kind by the modulus of the difference."""
    assert sum_d.shape == m["sum_d"].shape and sum_d.dtype == m["sum_d"].dtype and sum_d2.dtype == np.float64
    assert np.isfinite(sum_d).all() and np.isfinite(sum_d2).all()
    return (float((np.abs(sum_d - m["sum_d"]) / m["tol_d"]).max()),
            float((np.abs(sum_d2 - m["sum_d2"]) / m["tol_d2"]).max()))


def assert_symmetry(sum_d, sum_d2, kind):
    """What the mirrored store owes, to the bit: 'imag' and 'angle' change sign across the diagonal (channels of
    different 32-wide tiles, and of the same tile as well), the complex kind is Hermitian, the sum of squares symmetric
    for every kind."""
    C = sum_d.shape[-1]
    off = ~np.eye(C, dtype=bool)
    dT = sum_d.transpose(0, 2, 1)
    if kind in ("imag", "angle"):
        assert np.array_equal(dT[:, off], -sum_d[:, off]), f"{kind}: the mirror does not change sign"
    elif kind == "complex":
        assert np.array_equal(dT.conj(), sum_d), "complex: sum_d is not Hermitian"
    assert np.array_equal(sum_d2.transpose(0, 2, 1), sum_d2), "sum_d2 is not symmetric"


def check(sum_d, sum_d2, m, kind, what):
    """Print the case's err/tol, then assert the bound and the symmetries."""
    ed, ed2 = err_over_tol(sum_d, sum_d2, m)
    print(f"{what}: g_max {m['g_max']:.1f} min|c| {m['c_min']:.2f}  err/tol sum_d {ed:.3f} sum_d2 {ed2:.3f}")
    assert ed <= 1.0 and ed2 <= 1.0, f"{what}: err/tol sum_d {ed:.3g}, sum_d2 {ed2:.3g}"
    assert_symmetry(sum_d, sum_d2, kind)
    return max(ed, ed2)
