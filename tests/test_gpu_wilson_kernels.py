"""K6 (csrc/granger.hip, granger_kernels.h, wilson_plus_kernel.h) on the device at every size class of its kernel
dispatch, against NumPy complex128 (oracle/spy_oracle.py or plain np.linalg).

granger.hip picks its kernels by the channel count n and the LDS per workgroup (160 KiB on the MI355X), through
csrc/granger_route.h; tests/test_granger_route.py holds the table of size classes and checks the route against it for
every n up to 512.

N below touches every row of that table from 48 up, and every ragged form of each: 48 / 63 (16-row blocks, ragged MFMA tiles),
65 / 100 (32-row blocks, ragged last block, ragged last Cholesky panel), 128 (two full 64-row blocks), 161 / 255
(ragged last 64-row block and Cholesky panel), 200 (32-row blocks, ragged last one), 257 (16-row blocks above 256,
the column Cholesky), 300 (ragged 64-row blocks with the column Cholesky).  profiles/wilson_dispatch_kernels.txt is
a kernel trace of this file that shows those kernels per size.

The building-block bounds are those of the emulator tests of the same kernels (tests/test_emu_kernels.py), the
end-to-end bounds those of test_wilson_granger_vs_oracle (tests/test_gpu_production.py).
"""
import numpy as np
import pytest

from oracle import spy_oracle as O
from parity import assert_parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = [48, 63, 65, 100, 128, 161, 200, 255, 257, 300]
NF = 9                  # bins of the stepped calls: a batch that is not a multiple of 8 (XCD-aware zgemm grid)
RTOL, NITER, COND_MAX, EPS_MAX = 5e-6, 100, 1e4, 1e-1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from syncopy_amd import backend
    backend.require_gpu()


@pytest.fixture(scope="module")
def prims():
    from syncopy_amd.connectivity.wilson_sharded import HipPrims
    return HipPrims()


# ------------------------------------------------------------------------------------------------ fixtures
def _var_factors(C, F, seed):
    """Transfer function H(f) = A(f)^-1 and noise covariance Sigma = L L^T of a random stable VAR(2) process on F rfft
    bins (the NumPy branch of tests/test_gpu_production.py's _var_csd, same random stream)."""
    rng = np.random.default_rng(seed)
    A1 = 0.5 * np.eye(C) + rng.normal(size=(C, C)) * (0.25 / np.sqrt(C))
    A2 = -0.6 * np.eye(C) + rng.normal(size=(C, C)) * (0.15 / np.sqrt(C))
    L = np.eye(C) + 0.1 * np.tril(rng.normal(size=(C, C)), -1)
    Sigma = L @ L.T
    w = np.pi * np.arange(F) / (F - 1)
    A = np.eye(C)[None] - A1[None] * np.exp(-1j * w)[:, None, None] - A2[None] * np.exp(-2j * w)[:, None, None]
    return np.linalg.inv(A), Sigma


def _var_csd(C, F, seed, floor=0.05):
    """S(f) = H(f) Sigma H(f)^H + floor, complex64 (what the ST stage hands to the AV stage)."""
    H, Sigma = _var_factors(C, F, seed)
    S = H @ Sigma[None] @ H.conj().transpose(0, 2, 1) + floor * np.eye(C)[None]
    S = 0.5 * (S + S.conj().transpose(0, 2, 1))
    return S.astype(np.complex64)


def _herm(a):
    return a.conj().transpose(0, 2, 1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _rel(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(a - b).max() / np.abs(b).max())


def _cond_ladder(csd128, cond_max=COND_MAX, eps_max=EPS_MAX, nsteps=15):
    """Every condition number O.regularize_csd evaluates on the way to its decision, as (eps, cond) pairs."""
    eye = np.eye(csd128.shape[1])
    out = [(0.0, np.linalg.cond(csd128).max())]
    if out[0][1] < cond_max:
        return out
    for eps in np.logspace(-10, np.log10(eps_max), nsteps):
        out.append((float(eps), np.linalg.cond(csd128 + eps * eye).max()))
        if out[-1][1] < cond_max:
            break
    return out


def _wilson_sf_counted(CSD, nIter=NITER, rtol=RTOL):
    """O.wilson_sf, statement for statement, that also returns the error of every iteration (their number is the
    iteration count) and the final psi over the full (mirrored) frequency axis."""
    nF = CSD.shape[0]
    eye = np.eye(CSD.shape[1])
    full = np.r_[CSD, CSD[nF - 2:0:-1].conj()]
    psi0 = O.psi0_initial(full)
    psi = np.tile(psi0, (nF, 1, 1))
    psi = np.r_[psi, psi[nF - 2:0:-1].conj()]
    U = np.linalg.cholesky(full)
    converged, err, errs = False, np.inf, []
    for _ in range(nIter):
        g = np.linalg.inv(psi) @ U
        g = g @ _herm(g)
        gp, gp0 = O.plus_operator(g + eye)
        S = np.triu(gp0)
        S = S - S.conj().T
        psi = psi @ (gp + S)
        psi0 = psi0 @ (gp0 + S)
        err = O.max_rel_err(full, psi @ _herm(psi))
        errs.append(err)
        if err < rtol:
            converged = True
            break
    Sigma = psi0 @ psi0.T
    H = psi @ np.linalg.inv(psi0)
    return H[:nF], Sigma, converged, err, errs, psi, full


# ------------------------------------------------------------------------------------------------ A: stepped ABI
@pytest.mark.parametrize("n", N)
def test_cond(prims, n):
    """spyhip_wilson_cond: A = widen(csd) + eps I bit for bit; the power-iteration estimate of max_f cond_2(A_f)
    against LAPACK's SVD."""
    csd = _var_csd(n, NF, seed=n)
    for eps in (0.0, 1e-3):
        A, c = prims.cond(_dev(csd), eps)
        ref = csd.astype(np.complex128) + eps * np.eye(n)
        assert np.array_equal(_host(A), ref), eps
        np.testing.assert_allclose(c, np.linalg.cond(ref).max(), rtol=1e-4)


def _init(prims, n):
    csd = _var_csd(n, NF, seed=n)
    A, _ = prims.cond(_dev(csd), 0.0)
    U, gpart = prims.init(A, 0, NF)
    return A, U, gpart


@pytest.mark.parametrize("n", N)
def test_init(prims, n):
    """spyhip_wilson_init: the Cholesky factor of every bin and gamma_0 (O.psi0_initial: bin 0 of the FFT over the
    mirrored frequency axis, real part, symmetrised)."""
    A, U, gpart = _init(prims, n)
    A, U, gpart = _host(A), _host(U), _host(gpart)
    np.testing.assert_allclose(U, np.linalg.cholesky(A), rtol=1e-10, atol=1e-10)
    assert np.all(np.triu(U, 1) == 0)
    full = np.r_[A, A[NF - 2:0:-1].conj()]
    g0 = np.fft.fft(full, axis=0)[0]
    g0 = np.real((g0 + g0.T.conj()) / 2)
    assert _rel(gpart, g0) <= 1e-12


@pytest.mark.parametrize("n", N)
def test_psi0(prims, n):
    """spyhip_wilson_psi0: chol(gamma_0)^T, tiled exactly over the bins."""
    _, _, gpart = _init(prims, n)
    gamma0 = _host(gpart)
    psi0, psi = prims.psi0(gpart.clone(), NF)
    psi0, psi = _host(psi0), _host(psi)
    np.testing.assert_allclose(psi0, np.linalg.cholesky(gamma0).T, rtol=1e-10, atol=1e-10)
    for f in range(NF):
        assert np.array_equal(psi[f], psi0), f


def _g_ref(psi, U):
    X = np.linalg.inv(psi) @ U
    return X @ _herm(X) + np.eye(psi.shape[1])


@pytest.mark.parametrize("n", N)
def test_g_diagonally_dominant(prims, n):
    """spyhip_wilson_g with the block inverse of the size class: (psi^-1 U)(psi^-1 U)^H + I.  U comes from
    spyhip_wilson_init, so it really is lower triangular (the product skips the zero rows above a column tile)."""
    _, U, _ = _init(prims, n)
    rng = np.random.default_rng(n + 1)
    psi = rng.normal(size=(NF, n, n)) + 1j * rng.normal(size=(NF, n, n)) + 3 * np.sqrt(n) * np.eye(n)
    g, tiny = prims.g(_dev(psi), U, pivoted=False)
    g = _host(g)
    assert not tiny
    assert _rel(g, _g_ref(psi, _host(U))) <= 1e-9


@pytest.mark.parametrize("n", N)
def test_g_tiny_pivot_and_pivoted_retry(prims, n):
    """psi = a Cholesky factor with its columns reversed: invertible and well conditioned, but every leading diagonal
    block is zero.  The block inverse must raise its flag (rc 1); the pivoted inverse must get it right."""
    _, U, _ = _init(prims, n)
    rng = np.random.default_rng(n + 2)
    X = rng.normal(size=(NF, n, n)) + 1j * rng.normal(size=(NF, n, n))
    psi = np.ascontiguousarray(np.linalg.cholesky(X @ _herm(X) + 0.5 * n * np.eye(n))[:, :, ::-1])
    assert np.linalg.cond(psi).max() < 5.0          # the 1e-9 below is then the kernels' bound, not NumPy's
    g, tiny = prims.g(_dev(psi), U, pivoted=False)
    assert tiny
    g, tiny = prims.g(_dev(psi), U, pivoted=True)
    assert not tiny
    assert _rel(_host(g), _g_ref(psi, _host(U))) <= 1e-9


@pytest.mark.parametrize("n", N)
def test_update(prims, n):
    """spyhip_wilson_update: psi (g+ + S), psi0 (g0 + S) with S = triu(g0) - triu(g0)^H, and max_rel_err(A, psi psi^H)
    of the updated psi."""
    rng = np.random.default_rng(n + 3)
    cplx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)       # noqa: E731
    psi, gp, g0, psi0, X = cplx(NF, n, n), cplx(NF, n, n), cplx(n, n), cplx(n, n), cplx(NF, n, n)
    A = X @ _herm(X) + n * np.eye(n)
    S = np.triu(g0) - np.triu(g0).conj().T
    psi_ref, psi0_ref = psi @ (gp + S), psi0 @ (g0 + S)
    psi_d, psi0_d = _dev(psi), _dev(psi0)
    err = prims.update(psi_d, _dev(gp), _dev(g0), psi0_d, _dev(A))
    assert _rel(_host(psi_d), psi_ref) <= 1e-12
    assert _rel(_host(psi0_d), psi0_ref) <= 1e-12
    np.testing.assert_allclose(err, O.max_rel_err(A, psi_ref @ _herm(psi_ref)), rtol=1e-10)


@pytest.mark.parametrize("n", N)
def test_finish(prims, n):
    """spyhip_wilson_finish on the true factors of the VAR fixture: psi0 = chol(Sigma), psi = H psi0 gives back H and
    Sigma, and the Granger causality of S = H Sigma H^H.  Again with the columns of psi0 reversed (psi0 psi0^T and
    psi psi0^-1 are unchanged), where the block inverse of psi0 meets zero diagonal blocks and invert_one must fall
    back to the pivoted kernel."""
    H, Sigma = _var_factors(n, NF, seed=n)
    S = H @ Sigma[None] @ _herm(H)
    S = 0.5 * (S + _herm(S))
    Gref = O.granger(S, H, Sigma)
    chol = np.linalg.cholesky(Sigma)
    for psi0 in (chol, chol[:, ::-1]):
        psi0 = np.ascontiguousarray(psi0).astype(np.complex128)
        psi = H @ psi0
        G, Hd, Sd = prims.finish(_dev(S), _dev(psi), _dev(psi0))
        assert _rel(_host(Hd), H) <= 1e-9
        assert _rel(_host(Sd), Sigma) <= 1e-12
        assert_parity(_host(G), Gref, what=f"G, n = {n}")


# ------------------------------------------------------------------------------------------------ B: spyhip_granger
def _oracle_granger(csd, niter=NITER):
    """O.regularize_csd + the counted O.wilson_sf + O.granger on the complex128 widening of the complex64 CSD."""
    csd128 = csd.astype(np.complex128)
    reg, factor, cn0 = O.regularize_csd(csd128, cond_max=COND_MAX, eps_max=EPS_MAX)
    reg = reg.astype(np.complex128)
    Ho, So, conv, err, errs, psi, full = _wilson_sf_counted(reg, nIter=niter)
    return dict(reg=reg, factor=factor, cn0=cn0, H=Ho, Sigma=So, converged=conv, err=err, errs=errs, psi=psi,
                full=full, ladder=_cond_ladder(csd128))


@pytest.mark.parametrize("n", N)
def test_granger_vs_oracle(n):
    """spyhip_granger at every size class against the oracle: regularisation (this fixture regularises at n = 257 and
    300, factor 0.0228), factors, causality, the reconstruction on the host in complex128, and the iteration count.
    The oracle's condition number is that of the complex128 widening, which is what the device estimates."""
    from syncopy_amd import backend
    F = 65 if n <= 161 else 33
    csd = _var_csd(n, F, seed=n)
    o = _oracle_granger(csd)
    # preconditions on the reference side: the 1e-4 estimate of the condition number cannot flip a decision of the
    # ladder, and rounding cannot move the iteration at which the error crosses rtol
    for eps, c in o["ladder"]:
        assert abs(c / COND_MAX - 1.0) > 0.01, (eps, c)
    assert o["converged"] and len(o["errs"]) >= 2
    for e in o["errs"][-2:]:
        assert not RTOL / 2 <= e <= 2 * RTOL, o["errs"][-2:]
    G, meta, H, Sigma = backend.granger(_dev(csd), want_factors=True)
    iters = backend.granger_stats()["iterations"]
    G, H, Sigma = _host(G), _host(H), _host(Sigma)
    assert meta["converged"] and meta["max rel. err"] < RTOL
    assert meta["reg. factor"] == o["factor"]
    np.testing.assert_allclose(meta["initial cond. num"], o["cn0"], rtol=1e-4)
    assert iters == len(o["errs"])
    assert O.max_rel_err(o["reg"], H @ Sigma @ _herm(H)) < 1e-5
    np.testing.assert_allclose(H, o["H"], rtol=2e-4, atol=2e-5 * np.abs(o["H"]).max())
    np.testing.assert_allclose(Sigma, o["Sigma"], rtol=2e-4, atol=2e-5 * np.abs(o["Sigma"]).max())
    np.testing.assert_allclose(G, O.granger(o["reg"], o["H"], o["Sigma"]), rtol=2e-3, atol=2e-4)


# ------------------------------------------------------------------------------------------------ C: out of iterations
@pytest.mark.parametrize("n,F,seed", [(70, 129, 25), (100, 65, 20)])
def test_unconverged_error_is_over_all_bins(n, F, seed, monkeypatch):
    """With F >= 64 and n >= 48 the loop checks convergence on every 8th bin first.  A CSD whose worst bin (13) is not
    in that subset, cut off after 10 iterations: the reported error must be the one over ALL bins, and the same as
    with the full check forced (SPYHIP_WILSON_FULL_CHECK).  The seeds leave a large error at entry (5, 7) of bin 13
    (1.17 and 0.149 in the oracle), not a small difference of large numbers: see the reference-side checks."""
    from syncopy_amd import backend
    csd = _var_csd(n, F, seed=seed).astype(np.complex128)
    a, b = 5, 7
    s = csd[13, a, b] * (1.0 - 1e-6)                  # a rank-1 PSD block that cancels all but 1e-6 of entry (a, b)
    csd[13, a, a] += abs(s)
    csd[13, b, b] += abs(s)
    csd[13, a, b] -= s
    csd[13, b, a] -= np.conj(s)
    csd = csd.astype(np.complex64)
    o = _oracle_granger(csd, niter=10)
    assert not o["converged"] and len(o["errs"]) == 10
    full, psi = o["full"], o["psi"]
    e = np.abs(full - psi @ _herm(psi)) / np.abs(full)
    L = full.shape[0]
    assert np.unravel_index(e.argmax(), e.shape) in ((13, a, b), (13, b, a), (L - 13, a, b), (L - 13, b, a))
    # bin 13 and its mirror image are two float64 evaluations of the same quantity with their own rounding: they agree
    # ten times closer than the bound the device is held to
    assert abs(e[13].max() - e[L - 13].max()) <= 1e-7 * o["err"]
    sub = e[:F:8].max()                               # what the subset check sees (bins 0, 8, 16, ...)
    assert sub < 0.5 * o["err"], (sub, o["err"])     # a device that reported the subset bound would miss
    dev = _dev(csd)
    G1, meta1, H1, S1 = backend.granger(dev, niter=10, want_factors=True)
    assert not meta1["converged"] and backend.granger_stats()["iterations"] == 10
    np.testing.assert_allclose(meta1["max rel. err"], o["err"], rtol=1e-6)
    monkeypatch.setenv("SPYHIP_WILSON_FULL_CHECK", "1")
    G2, meta2, H2, S2 = backend.granger(dev, niter=10, want_factors=True)
    assert meta2 == meta1 and backend.granger_stats()["iterations"] == 10
    for x, y in ((G1, G2), (H1, H2), (S1, S2)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ D: plus operator
@pytest.mark.parametrize("nftot,nent", [(18, 9), (33, 9), (129, 9), (2049, 9), (4097, 9), (2501, 9), (3001, 9),
                                        (8193, 9), (8193, 2116)])
def test_plus_operator(prims, nftot, nent):
    """spyhip_wilson_plus against O.plus_operator, on random complex g (complex DC and Nyquist bins: their imaginary
    parts must be ignored).  Lag-domain length L = 2 (nftot - 1): 34 radix-17 pass, 64 generic LDS kernel, 256 / 4096
    plus4<8> / plus4<12> (nent = 9 leaves a ragged quad), 5000 radix-5 generic, 6000 / 8192 / 16384 plus_long_kernel
    (two length-L arrays exceed LDS); 2116 entries at 16384 take two launches of that kernel (2048 + 68 entries)."""
    rng = np.random.default_rng(nftot + nent)
    g = rng.normal(size=(nftot, nent)) + 1j * rng.normal(size=(nftot, nent))
    gp, g0 = prims.plus(_dev(g))
    gp, g0 = _host(gp), _host(g0)
    L = 2 * (nftot - 1)
    for e0 in range(0, nent, 256):                    # the oracle entry by entry in slices (1-2 GB at once otherwise)
        sl = slice(e0, min(e0 + 256, nent))
        full = np.empty((L, sl.stop - sl.start), complex)
        full[:nftot] = g[:, sl]
        full[nftot:] = np.conj(g[1:nftot - 1, sl][::-1])
        ref, ref0 = O.plus_operator(full)
        np.testing.assert_allclose(gp[:, sl], ref[:nftot], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(g0[sl], ref0, rtol=1e-12, atol=1e-12)
