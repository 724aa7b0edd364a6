"""Float64 NumPy model of the directed measures of the Wilson factors (TEST INFRASTRUCTURE ONLY): the directed transfer
function and partial directed coherence with their noise-weighted forms (directed coherence, generalised PDC), the
kernel-level form of syncopy_amd/csrc/directed_kernel.h, the chain model from a trial-averaged CSD (oracle.spy_oracle's
regularize_csd and wilson_sf, as its granger_cF calls them), and the bounds the tests hold the kernels to.

Layout throughout: [f, sender, receiver]; H[f, r, s] carries the noise of channel s into channel r; A = H^-1."""
import numpy as np

from oracle import spy_oracle as O

U32 = 2.0 ** -24            # unit roundoff of float32
U64 = 2.0 ** -53
SHAPES = [(1, 2), (3, 5), (2, 63), (2, 64), (2, 65), (1, 256), (1, 257)]        # (F, n) of the kernel tests
MEASURES = ("dtf", "pdc")


def _safe_div(num, den):
    """num / den, 0 where den is 0"""
    out = np.zeros(np.broadcast(num, den).shape)
    np.divide(num, den, out=out, where=den > 0)
    return out


def dtf(H, Sigma=None, output="abs"):
    """dtf[f,s,r] = sigma_s |H[f,r,s]| / sqrt(sum_k sigma_k^2 |H[f,r,k]|^2); Sigma=None: every sigma is 1"""
    sig = np.ones(H.shape[1]) if Sigma is None else np.sqrt(np.real(np.diagonal(Sigma)))
    a = np.abs(H.astype(np.complex128)) * sig[None, None, :]                    # [f, r, s]
    res = _safe_div(a, np.sqrt((a ** 2).sum(axis=2, keepdims=True))).transpose(0, 2, 1)
    return res ** 2 if output == "pow" else res


def pdc(H, Sigma=None, output="abs"):
    """pdc[f,s,r] = |A[f,r,s]| / sigma_r / sqrt(sum_k |A[f,k,s]|^2 / sigma_k^2) with A = H^-1"""
    return pdc_of_inverse(np.linalg.inv(H.astype(np.complex128)), Sigma, output)


def pdc_of_inverse(A, Sigma=None, output="abs"):
    sig = np.ones(A.shape[1]) if Sigma is None else np.sqrt(np.real(np.diagonal(Sigma)))
    a = np.abs(A) / sig[None, :, None]                                          # [f, r, s]
    res = _safe_div(a, np.sqrt((a ** 2).sum(axis=1, keepdims=True))).transpose(0, 2, 1)
    return res ** 2 if output == "pow" else res


def directed_norm(M, w=None, axis=0, squared=False):
    """spyhip_directed_norm (include/spyhip.h) in float64"""
    w = np.ones(M.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    a = np.abs(M.astype(np.complex128))
    if axis == 0:
        a = a * w[None, None, :]
        res = _safe_div(a, np.sqrt((a ** 2).sum(axis=2, keepdims=True)))
    else:
        a = a * w[None, :, None]
        res = _safe_div(a, np.sqrt((a ** 2).sum(axis=1, keepdims=True)))
    res = res.transpose(0, 2, 1)
    return res ** 2 if squared else res


def matrices(F, n, seed=0, dead=False):
    """complex128 (F, n, n) test matrices; dead: row 1 and column 0 are exactly zero (n >= 2)"""
    rng = np.random.default_rng([seed, F, n])
    M = rng.normal(size=(F, n, n)) + 1j * rng.normal(size=(F, n, n))
    M *= np.exp(rng.uniform(-3, 3, size=(F, n, n)))                             # magnitudes over some decades
    if dead:
        M[:, 1, :] = 0
        M[:, :, 0] = 0
    return M


def weights(n, seed=0):
    return np.exp(np.random.default_rng([seed, n, 7]).uniform(-1, 1, size=n))


def well_conditioned(batch, n, seed=0):
    """I + 0.3 G / sqrt(n) with complex Gaussian G: condition numbers below 1e2"""
    rng = np.random.default_rng([seed, batch, n, 3])
    G = rng.normal(size=(batch, n, n)) + 1j * rng.normal(size=(batch, n, n))
    return np.eye(n)[None] + 0.3 * G / np.sqrt(n)


def residual(M, X):
    """max |M X - I| per matrix"""
    return np.abs(M @ X - np.eye(M.shape[1])[None]).reshape(M.shape[0], -1).max(axis=1)


def inverse_bound(M):
    """what spyhip_zinv may leave of max |M X - I| per matrix: 8 times the residual of NumPy's own LAPACK inverse plus
    n 2^-52 cond(M) - the margin is for the unpivoted block order of the matrix-core kernels"""
    n = M.shape[1]
    return 8 * residual(M, np.linalg.inv(M)) + n * 2.0 ** -52 * np.linalg.cond(M)


def pdc_bound(M, w=None):
    """Bound of |pdc(X) - pdc(M^-1)| for an X within inverse_bound of the inverse, per element [f, s, r], from the model
    alone.  M X = I + R with max |R| <= rho gives X = A (I + R), A = M^-1: column s of X differs from column s of A by
    A R[:, s], at most rho * sum_k |A[r, k]| in row r.  With weighted columns a = w_r |A[r, s]|, the value a_r / ||a||
    moves by at most 2 ||delta|| / ||a|| (the numerator moves by delta_r, the norm by at most ||delta||, and the value is
    at most 1), ||delta|| being the 2-norm of the weighted perturbation of the column.  Plus the float32 rounding."""
    A = np.linalg.inv(M)
    w = np.ones(M.shape[1]) if w is None else np.asarray(w)
    rho = inverse_bound(M)                                                       # (F,)
    delta = rho[:, None] * np.abs(A).sum(axis=2) * w[None, :]                    # (F, r): any column
    dnorm = np.sqrt((delta ** 2).sum(axis=1))                                    # (F,)
    colnorm = np.sqrt(((np.abs(A) * w[None, :, None]) ** 2).sum(axis=1))         # (F, s)
    return U32 + 2 * (dnorm[:, None] / colnorm)[:, :, None] * np.ones((1, 1, M.shape[1]))


def chain(csd, rtol=5e-6, nIter=100, cond_max=1e4):
    """The float64 chain model on a trial-averaged CSD (F, C, C): (H, Sigma, info) as oracle.spy_oracle.granger_cF forms them"""
    reg, factor, cn0 = O.regularize_csd(np.asarray(csd), cond_max=cond_max, eps_max=1e-1)
    H, Sigma, conv, err = O.wilson_sf(reg.astype(np.complex128), nIter=nIter, rtol=rtol)
    return H, Sigma, {"converged": bool(conv), "max rel. err": float(err), "reg. factor": factor, "initial cond. num": float(cn0)}


def measure(method, H, Sigma, noise_weighted=False, output="abs"):
    return (dtf if method == "dtf" else pdc)(H, Sigma if noise_weighted else None, output)


# ---- the chain model as a routine of the front end -------------------------------------------------------------------------
_chains = {}


def cached_chain(csd, rtol=5e-6, nIter=100, cond_max=1e4):
    """chain() once per CSD: the tests ask for several measures of one factorisation"""
    csd = np.ascontiguousarray(csd)
    key = (csd.tobytes(), csd.shape, str(csd.dtype), rtol, nIter, cond_max)
    if key not in _chains:
        _chains[key] = chain(csd, rtol, nIter, cond_max)
    return _chains[key]


def directed_cF(csd_av, method="dtf", noise_weighted=False, output="abs", rtol=5e-6, nIter=100, cond_max=1e4,
                chunkShape=None, noCompute=False):
    if noCompute:
        return csd_av.shape, np.float32
    H, Sigma, info = cached_chain(csd_av[0], rtol, nIter, cond_max)
    meta = {"converged--bool": np.array(info["converged"]), "max rel. err--float": np.array(info["max rel. err"]),
            "reg. factor--float": np.array(info["reg. factor"]), "initial cond. num--float": np.array(info["initial cond. num"])}
    return measure(method, H, Sigma, noise_weighted, output)[None, ...], meta


def oracle_classes():
    """routine_classes that run 'dtf' / 'pdc' (and every stage under them) on the CPU model"""
    from oracle_routines import ORACLE_CONN, OracleGrangerCausality

    class OracleDirectedMeasure(OracleGrangerCausality):
        computeFunction = staticmethod(directed_cF)

    return {**ORACLE_CONN, "dtf": OracleDirectedMeasure, "pdc": OracleDirectedMeasure}
