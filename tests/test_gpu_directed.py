"""The directed measures on the device: spyhip_directed_norm at the shapes of tests/directed_oracle.py under the float32
rounding bound, spyhip_zinv at one size per inverse class of tests/test_granger_route.py against NumPy's LAPACK inverse,
the two chained as the PDC is, and `spy.connectivityanalysis(method="dtf" | "pdc")` from AnalogData and SpectralData
against the float64 chain model.  Every comparison prints its err/tol (pytest -s)."""
import numpy as np
import pytest

import directed_oracle as DO
import syncopy_amd as spy
from oracle_routines import ORACLE_FREQ

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


# ---- spyhip_directed_norm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DO.SHAPES + [(9, 40), (2, 320)], ids=lambda s: "-".join(map(str, s)))
def test_directed_norm(be, shape):
    """the shapes of the emulator test, nine matrices (two rounds of the 8 XCD slots) and a strip that does not fit LDS"""
    F, n = shape
    M, w = DO.matrices(F, n, dead=n >= 5), DO.weights(n)
    Md, wd = _dev(M), _dev(w)
    worst = 0.0
    for axis in (0, 1):
        for weights, wdev in ((None, None), (w, wd)):
            for squared in (False, True):
                got = be.directed_norm(Md, wdev, axis, squared).cpu().numpy()
                want = DO.directed_norm(M, weights, axis, squared)
                err = np.abs(got.astype(np.float64) - want).max()
                worst = max(worst, err / DO.U32)
                assert np.isfinite(got).all() and err <= DO.U32, (shape, axis, weights is not None, squared, err / DO.U32)
                if n >= 5:      # receiver 1 (a zero row of M) and sender 0 (a zero column): 0, not NaN
                    assert np.all(got[:, :, 1] == 0) and np.all(got[:, 0, :] == 0)
                if squared:
                    total = got.astype(np.float64).sum(axis=1 if axis == 0 else 2)
                    alive = want.sum(axis=1 if axis == 0 else 2) > 0.5
                    assert np.abs(total[alive] - 1).max() <= n * DO.U32 and np.all(total[~alive] == 0)
    print(f"directed_norm {shape}: worst err/tol {worst:.3f}")
    assert torch.equal(Md, _dev(M))                                   # the input is left alone


def test_directed_norm_numpy_host(be):
    """the torch-free binding"""
    from syncopy_amd import abi
    dev = abi.Device(0)
    M, w = DO.matrices(3, 5), DO.weights(5)
    try:
        for axis in (0, 1):
            got = dev.directed_norm(M, w, axis=axis, squared=True)
            assert got.dtype == np.float32 and np.abs(got - DO.directed_norm(M, w, axis, True)).max() <= DO.U32
        X = dev.zinv(DO.well_conditioned(2, 5))
        assert np.all(DO.residual(DO.well_conditioned(2, 5), X) <= DO.inverse_bound(DO.well_conditioned(2, 5)))
    finally:
        dev.close()


# ---- spyhip_zinv ----------------------------------------------------------------------------------------------------------------
ZINV = [(3, 5), (3, 40), (9, 40), (3, 100), (3, 200), (3, 256)]        # pivoted, 16-row blocks, 32-row and 64-row matrix-core blocks


@pytest.mark.parametrize("batch,n", ZINV, ids=lambda v: str(v))
def test_zinv(be, batch, n):
    M = DO.well_conditioned(batch, n)
    assert np.linalg.cond(M).max() < 1e2
    tol = DO.inverse_bound(M)
    Md = _dev(M)
    out = be.zinv(Md)
    assert torch.equal(Md, _dev(M)) and out.data_ptr() != Md.data_ptr()
    r_out = DO.residual(M, out.cpu().numpy())
    same = be.zinv(Md, out=Md)
    assert same is Md
    r_in = DO.residual(M, Md.cpu().numpy())
    print(f"zinv {batch} x {n}: worst residual/tol {max((r_out / tol).max(), (r_in / tol).max()):.3f}")
    assert np.all(r_out <= tol) and np.all(r_in <= tol)
    assert np.array_equal(out.cpu().numpy(), Md.cpu().numpy())        # in place and out of place are the same arithmetic


@pytest.mark.parametrize("n", [40, 100, 256])
def test_zinv_repeats_with_pivoting(be, n):
    """the anti-diagonal permutation of tests/test_emu_kernels.py::test_blocked_inverse - every leading diagonal block
    is singular - between two well-conditioned matrices: the block kernel flags it, the pivoted kernel inverts all three"""
    M = DO.well_conditioned(3, n, seed=5)
    M[1] = np.eye(n)[::-1]
    tol = DO.inverse_bound(M)
    for in_place in (False, True):
        Md = _dev(M)
        X = be.zinv(Md, out=Md if in_place else None).cpu().numpy()
        res = DO.residual(M, X)
        print(f"zinv pivoted repeat n = {n}{' in place' if in_place else ''}: worst residual/tol {(res / tol).max():.3f}")
        assert np.all(res <= tol) and np.array_equal(X[1], np.eye(n)[::-1])


@pytest.mark.parametrize("n", [5, 40, 100])
def test_zinv_singular(be, n):
    """an exactly singular matrix (a zero column) is an error of the call, and the context goes on working"""
    from syncopy_amd._lib import SpyHipError
    M = DO.well_conditioned(3, n, seed=7)
    M[2, :, n // 2] = 0
    with pytest.raises(SpyHipError, match="singular"):
        be.zinv(_dev(M))
    good = DO.well_conditioned(3, n, seed=7)
    assert np.all(DO.residual(good, be.zinv(_dev(good)).cpu().numpy()) <= DO.inverse_bound(good))


# ---- PDC at kernel level ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,n", ZINV, ids=lambda v: str(v))
def test_pdc_from_the_inverse(be, batch, n):
    M, w = DO.well_conditioned(batch, n, seed=11), DO.weights(n, seed=11)
    worst = 0.0
    for weights in (None, w):
        Md = _dev(M)
        be.zinv(Md, out=Md)
        got = be.directed_norm(Md, None if weights is None else _dev(weights), axis=1).cpu().numpy()
        want = DO.pdc_of_inverse(np.linalg.inv(M)) if weights is None else DO.directed_norm(np.linalg.inv(M), weights, 1)
        ratio = np.abs(got - want) / DO.pdc_bound(M, weights)
        worst = max(worst, ratio.max())
        assert ratio.max() <= 1, (batch, n, weights is not None, ratio.max())
    print(f"pdc of zinv {batch} x {n}: worst err/tol {worst:.3f}")


# ---- the front end ------------------------------------------------------------------------------------------------------------------
# With AnalogData the ST stage demeans every tapered trial (granger's rule), so the DC bin of the trial-averaged cross
# spectra is the transform's rounding residue: a matrix of no fixed direction, 14 decades below its neighbours - and the
# factorisation, which works along the whole frequency axis, is sensitive to that direction.  On the CPU, the chain model
# of one CSD against the chain model of the same CSD with another random matrix in its DC bin differs by up to 3.5 times
# this file's bound in every bin (the Granger values of the same two factorisations stay inside it above the lowest bins:
# they are quadratic in the small entries of H, dtf and pdc linear).  The device's residue is not the oracle routines'.
# So the chain model factorises the trial-averaged cross spectra the device's own ST stage formed - that stage is compared
# with its oracle elsewhere (test_gpu_golden.py, test_gpu_edge.py) - and every bin is held to the bound, DC included; the
# distance to the model run on the oracle's ST stage is printed.  SpectralData input carries no such bin: there the model
# runs from the same spectra through its own stages.
COMBOS = [(m, nw, out) for m in DO.MEASURES for nw in (False, True) for out in ("abs", "pow")]
INFO = {"converged", "max rel. err", "reg. factor", "initial cond. num"}


@pytest.fixture(scope="module")
def small():
    adj = np.zeros((4, 4))
    adj[0, 1], adj[2, 3] = 0.25, 0.2
    return spy.synthdata.ar2_network(AdjMat=adj, nSamples=500, nTrials=40, seed=3, samplerate=1000)


def _model(data, **kw):
    return spy.connectivityanalysis(data, compute_method="sequential", routine_classes=DO.oracle_classes(), **kw)


def _over_tol(got, want):
    return (np.abs(got - want) / (2e-4 + 2e-3 * np.abs(want))).max()


def _with_device_csd(data, **kw):
    """(result, trial-averaged cross spectra the AV stage was handed) of one batched call"""
    from syncopy_amd.connectivity.AV_compRoutines import DirectedMeasure
    keep = {}

    class Keep(DirectedMeasure):
        def compute_hip(self, st_out, out):
            keep["csd"] = self._device_input(st_out)[0].cpu().numpy()
            super().compute_hip(st_out, out)

    got = spy.connectivityanalysis(data, routine_classes={kw["method"]: Keep}, **kw)
    return got, keep["csd"]


@pytest.mark.parametrize("method,noise_weighted,output", COMBOS, ids=lambda v: str(v))
def test_front_end_from_analog_data(be, small, method, noise_weighted, output):
    kw = dict(method=method, noise_weighted=noise_weighted, output=output, tapsmofrq=5)
    got, csd = _with_device_csd(small, **kw)
    plain = spy.connectivityanalysis(small, **kw)
    assert np.array_equal(plain.data, got.data) and plain.info == got.info
    H, Sigma, info = DO.cached_chain(csd)
    want = DO.measure(method, H, Sigma, noise_weighted, output)
    assert got.data.dtype == np.float32 and got.data.shape == (1, 251, 4, 4) and set(got.info) == INFO
    assert got.info["converged"] is True and info["converged"]
    assert list(got.channel_i) == list(small.channel) == list(got.channel_j) and np.array_equal(got.freq, np.fft.rfftfreq(500, 1e-3))
    ref = _model(small, **kw)
    print(f"AnalogData {method} {noise_weighted} {output}: worst err/tol {_over_tol(got.data[0], want):.3f}; "
          f"against the model on the oracle's ST stage {_over_tol(got.data, ref.data):.1f}, from bin 2 on {_over_tol(got.data[:, 2:], ref.data[:, 2:]):.2f}")
    np.testing.assert_allclose(got.data[0], want, rtol=2e-3, atol=2e-4)       # test_gpu_golden.py::test_conn5_granger's bound
    if output == "pow":
        assert np.allclose(got.data[0].sum(axis=1 if method == "dtf" else 2), 1, atol=4 * DO.U32)
    seq = spy.connectivityanalysis(small, compute_method="sequential", **kw)   # the same device path per call
    assert seq.info["converged"] is True
    print(f"  sequential against batched: worst err/tol {_over_tol(seq.data[:, 2:], got.data[:, 2:]):.3f} from bin 2 on")


@pytest.fixture(scope="module")
def small_spectra(small):
    return spy.freqanalysis(small, method="mtmfft", output="fourier", keeptapers=True, tapsmofrq=5,
                            compute_method="sequential", routine_classes=ORACLE_FREQ)


@pytest.mark.parametrize("method,noise_weighted,output", COMBOS, ids=lambda v: str(v))
def test_front_end_from_spectral_data(be, small_spectra, method, noise_weighted, output):
    kw = dict(method=method, noise_weighted=noise_weighted, output=output)
    got = spy.connectivityanalysis(small_spectra, **kw)
    ref = _model(small_spectra, **kw)
    assert got.data.dtype == np.float32 and got.data.shape == ref.data.shape and set(got.info) == INFO
    assert got.info["converged"] is True and ref.info["converged"] is True
    assert list(got.channel_i) == list(ref.channel_i) and np.array_equal(got.freq, ref.freq)
    print(f"SpectralData {method} {noise_weighted} {output}: worst err/tol {_over_tol(got.data, ref.data):.3f}")
    np.testing.assert_allclose(got.data, ref.data, rtol=2e-3, atol=2e-4)
    if (noise_weighted, output) == (False, "abs"):
        send, rec = [3, 0], [1, 2, 3]
        part = spy.connectivityanalysis(small_spectra, channelcmb=[send, rec], **kw)
        assert part.data.shape == got.data.shape[:2] + (2, 3) and part.info == got.info
        assert np.array_equal(part.data, got.data[:, :, send, :][:, :, :, rec])
        assert list(part.channel_i) == list(np.array(got.channel_i)[send]) and list(part.channel_j) == list(np.array(got.channel_j)[rec])


def test_front_end_at_a_matrix_core_size(be):
    """65 channels x 256 samples x 700 trials: matrix-core products, the 32-row block inverse, one channel into the third
    strip of the finalizer.  The model factorises the device's cross spectra once for the four results (both reach a
    relative error of 5.1e-8: measured on an MI355X, device 5.06e-08, model 5.07e-08, worst err/tol of the measures 0.000)."""
    adj = np.zeros((65, 65))
    for i in range(0, 64, 8):
        adj[i, i + 1] = 0.2
    data = spy.synthdata.ar2_network(AdjMat=adj, nSamples=256, nTrials=700, seed=65, samplerate=1000)
    for method in DO.MEASURES:
        for nw in (False, True):
            got, csd = _with_device_csd(data, method=method, noise_weighted=nw, tapsmofrq=8)
            H, Sigma, info = DO.cached_chain(csd)
            want = DO.measure(method, H, Sigma, nw)
            assert got.data.shape == (1, 129, 65, 65) and got.info["converged"] == info["converged"]
            print(f"65 channels {method} {nw}: worst err/tol {_over_tol(got.data[0], want):.3f}, "
                  f"max rel. err device {got.info['max rel. err']:.2e} model {info['max rel. err']:.2e}")
            np.testing.assert_allclose(got.data[0], want, rtol=2e-3, atol=2e-4)
