"""The phase slope index on the device: K13 (phaseslope_kernel) at the kernel shapes of tests/psi_oracle.py against its
float64 model under its bound, and `spy.connectivityanalysis(method="psi")` from AnalogData, from SpectralData and through
the torch-free host against the model applied to the complex coherence of the same call.  Every comparison prints its
err/tol (pytest -s)."""
import warnings

import numpy as np
import pytest

import psi_oracle as PO
import syncopy_amd as spy
from parity import ATOL_REL, RTOL, excess, jackknife_tolerances
from syncopy_amd.shared.errors import SPYValueError

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.fixture(scope="module")
def cases(be):
    """per (channels, frequencies): the CSD and K5's coherency of it on the device, computed once"""
    out = {}
    for Cn, F, _ in PO.SHAPES:
        if (Cn, F) not in out:
            csd = PO.hermitian_csd(PO.spectra(Cn, F))
            out[Cn, F] = csd, be.coh_normalize(_dev(csd), "complex").cpu().numpy()
    return out


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernel_shapes(be, cases, shape):
    Cn, F, half = shape
    csd, coh = cases[Cn, F]
    got = be.phase_slope(_dev(csd), half).cpu().numpy()
    PO.check(got, coh, half, what="device " + "-".join(map(str, shape)))
    valid = slice(half, F - half) if half else slice(0, 1)
    assert not got[valid, -1, :].any() and not got[valid, :, -1].any()               # the zero channel: exact zeros
    if Cn == 1:
        assert not got[valid].any()
    else:
        assert np.abs(got[valid, :Cn - 1, :Cn - 1]).max() > 0.05                     # not noise
    # the two entries agree bit for bit; the strictly upper tiles of the accumulator are NaN and are not read
    raw = PO.raw_accumulator(csd)
    acc = _dev(raw)
    again = be.phase_slope_from_accumulator(acc, PO.SCALE, half).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), raw.view(np.uint32))    # not modified


def test_half_zero_leaves_the_rest_of_out_alone(be, cases):
    csd, coh = cases[33, 41]
    ctx = be.context()
    ctx.bind_stream()
    d, out = _dev(csd), torch.full((3, 33, 33), 7.5, dtype=torch.float32, device="cuda")
    assert ctx.lib.spyhip_phaseslope(ctx.handle, d.data_ptr(), 41, 33, 0, out.data_ptr()) == 0
    got = out.cpu().numpy()
    assert np.all(got[1:] == 7.5)
    PO.check(got[:1], coh, 0, what="device 33-41-0, three planes given")


def test_refusals(be, cases):
    csd, _ = cases[33, 9]
    d = _dev(csd)
    assert np.isfinite(be.phase_slope(d, 4).cpu().numpy()[4]).all()                  # 2h = F - 1 fits: one valid bin
    ctx = be.context()
    out = torch.full((9, 33, 33), 3.5, dtype=torch.float32, device="cuda")
    p, o = d.data_ptr(), out.data_ptr()
    for fn, scale in ((ctx.lib.spyhip_phaseslope, ()), (ctx.lib.spyhip_phaseslope_from_accumulator, (1.0,))):
        for args in ((None, p, 9, 33, *scale, 1, o), (ctx.handle, None, 9, 33, *scale, 1, o), (ctx.handle, p, 9, 33, *scale, 1, None),
                     (ctx.handle, p, 0, 33, *scale, 1, o), (ctx.handle, p, 1, 33, *scale, 0, o), (ctx.handle, p, 9, 0, *scale, 1, o),
                     (ctx.handle, p, 9, -3, *scale, 1, o), (ctx.handle, p, 9, 33, *scale, -1, o), (ctx.handle, p, 9, 33, *scale, 5, o),
                     (ctx.handle, p, 2, 33, *scale, 1, o)):
            assert fn(*args) == -1, args
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 3.5)
    with pytest.raises(be.SpyHipError):
        be.phase_slope(d, 5)
    with pytest.raises(be.SpyHipError):
        be.phase_slope_from_accumulator(d, 1.0, -1)


def test_entries_are_in_the_library(be):
    from syncopy_amd import _lib
    for fn in ("spyhip_phaseslope", "spyhip_phaseslope_from_accumulator"):
        assert fn in _lib.SIGNATURES and hasattr(_lib.load(), fn)


# ---- the front end --------------------------------------------------------------------------------------------------------------
KW = dict(tapsmofrq=10, foilim=[10, 60])
BW, H, NF = 8, 4, 51                       # df = 1 Hz: h = round(8 / 2) = 4 bins, 51 frequencies, valid bins 4 ... 46
VALID = slice(H, NF - H)
# the arithmetic the front end gives psi, asked for by name so that the coherence of the comparison is formed from the very
# same cross spectra: float64 transforms, and (below) K4's directly summed imaginary parts, as for coh with output="imag",
# with every trial's cross spectrum accumulated on its own and the trials added in float64 (backend.csd_trials_apart)
SAME = dict(precision="reference")


@pytest.fixture(scope="module")
def coupled():
    """the delayed-copies recording of tests/test_gpu_pair_kernels.py::coupled_data: 5 trials of 1 s at 1 kHz, 33 channels, a
    common broadband signal that reaches channel c (c % 4) samples after the channels with c % 4 == 0"""
    rng = np.random.default_rng(1933)
    ntr, n, C = 5, 1000, 33
    common = rng.normal(size=ntr * n + 3)
    x = 0.6 * rng.normal(size=(ntr * n, C))
    for c in range(C):
        x[:, c] += 1.5 * common[3 - c % 4:3 - c % 4 + ntr * n]
    trl = np.stack([np.arange(ntr) * n, np.arange(1, ntr + 1) * n, np.zeros(ntr)], axis=1)
    return spy.AnalogData(x.astype(np.float32), samplerate=1000.0, trialdefinition=trl)


def _coherency(be, obj, **kw):
    """connectivityanalysis(method="coh", output="complex") in the arithmetic of psi"""
    with be.csd_phase_exact(True), be.csd_trials_apart(True):
        return np.asarray(spy.connectivityanalysis(obj, method="coh", output="complex", **kw).data[0])


@pytest.fixture(scope="module")
def square(be, coupled):
    """psi of the recording, and the complex coherence of the same call"""
    res = spy.connectivityanalysis(coupled, method="psi", bandwidth=BW, **KW, **SAME)
    return res, _coherency(be, coupled, **KW, **SAME)


def test_from_analog_data(be, coupled, square):
    res, coh = square
    assert isinstance(res, spy.CrossSpectralData) and res.data.dtype == np.float32 and res.data.shape == (1, NF, 33, 33)
    assert res.freq[0] == 10 and res.freq[-1] == 60 and list(res.channel_i) == list(coupled.channel)
    cfg = res.cfg["connectivityanalysis"]
    assert cfg["method"] == "psi" and cfg["bandwidth"] == BW and cfg["h"] == H
    PO.check(np.asarray(res.data[0]), coh, H, what="front end, AnalogData")
    # the sign: the channels with c % 4 == 0 lead those with c % 4 == 3, in every valid bin
    assert np.all(res.data[0, VALID, 0, 3] > 0) and np.all(res.data[0, VALID, 3, 0] < 0)
    print("psi[valid, 0, 3]: min %.3g mean %.3g" % (res.data[0, VALID, 0, 3].min(), res.data[0, VALID, 0, 3].mean()))
    # the default precision ("auto") takes the same float64 transforms and exact imaginary parts on its own
    auto = spy.connectivityanalysis(coupled, method="psi", bandwidth=BW, **KW)
    assert np.array_equal(np.asarray(auto.data), np.asarray(res.data), equal_nan=True)
    # ... which the complex coherence of a default call does not (float32 transforms, three-multiplication products): for
    # the record, how far psi is from the model on THAT coherence, in units of the kernel bound
    plain = np.asarray(spy.connectivityanalysis(coupled, method="coh", output="complex", **KW).data[0])
    m = PO.psi_model(plain, H)[VALID]
    print("against the coherence of a default call: err/bound %.3g" % (np.abs(res.data[0, VALID] - m) / PO.bound(m, NF, H)).max())


def test_whole_axis(be, coupled, square):
    res = spy.connectivityanalysis(coupled, method="psi", **KW, **SAME)
    assert res.data.shape == (1, 1, 33, 33) and list(res.freq) == [35.0]
    assert res.cfg["connectivityanalysis"]["h"] == 0 and "bandwidth" not in res.cfg["connectivityanalysis"]
    PO.check(np.asarray(res.data[0]), square[1], 0, what="front end, whole axis")
    assert res.data[0, 0, 0, 3] > 0 > res.data[0, 0, 3, 0]


@pytest.fixture(scope="module")
def spectra(coupled):
    return spy.freqanalysis(coupled, method="mtmfft", output="fourier", keeptapers=True, keeptrials=True, **KW, **SAME)


def test_from_spectral_data_and_channelcmb(be, spectra):
    res = spy.connectivityanalysis(spectra, method="psi", bandwidth=BW)
    assert res.data.shape == (1, NF, 33, 33) and res.data.dtype == np.float32
    PO.check(np.asarray(res.data[0]), _coherency(be, spectra), H, what="front end, SpectralData with kept tapers")
    assert np.all(res.data[0, VALID, 0, 3] > 0) and np.all(res.data[0, VALID, 3, 0] < 0)
    cmb = spy.connectivityanalysis(spectra, method="psi", bandwidth=BW, channelcmb=[[0, 1], [3, 7]])
    assert cmb.data.shape == (1, NF, 2, 2) and cmb.cfg["connectivityanalysis"]["h"] == H
    assert list(cmb.channel_i) == list(spectra.channel[[0, 1]]) and list(cmb.channel_j) == list(spectra.channel[[3, 7]])
    assert np.array_equal(np.asarray(cmb.data), np.asarray(res.data)[..., [0, 1], :][..., [3, 7]], equal_nan=True)


def test_sequential_route(coupled, square):
    """the per-trial engine accumulates the cross spectra trial by trial and hands them to the same AV class.
    Measured on an MI355X: err/tol 0.35.  Both routes take float64 transforms and K4's exact imaginary parts, and the
    batched route sums every trial's 19 rows on their own and the trials in float64 (backend.csd_trials_apart), so that
    the routes differ by the engine's scaling and its complex64 sum over trials on the host.  With one float32 chain over
    all 95 rows on the batched route the figure was 1.30: psi, a sum of products of unit-scale coherencies that is 0.24
    at the most here, inherits about 1e-7 from the chain while the criterion allows 2.4e-7 where psi is small."""
    seq = spy.connectivityanalysis(coupled, method="psi", bandwidth=BW, compute_method="sequential", **KW)
    got, ref = np.asarray(seq.data[0]), np.asarray(square[0].data[0])
    assert got.shape == ref.shape and np.isnan(got[:H]).all() and np.isnan(got[NF - H:]).all()
    e = excess(got[VALID], ref[VALID])
    print(f"sequential against batched: err/tol {e:.3g}")
    assert e <= 1.0, e


def test_rules(coupled, spectra):
    for obj in (coupled, spectra):
        kw = KW if obj is coupled else {}
        with pytest.raises(SPYValueError, match="trial averaging needed for method psi"):
            spy.connectivityanalysis(obj, method="psi", keeptrials=True, **kw)
        with pytest.raises(SPYValueError, match="only one trial"):
            spy.connectivityanalysis(obj, method="psi", select={"trials": [2]}, **kw)
        with pytest.raises(SPYValueError, match="bandwidth"):
            spy.connectivityanalysis(obj, method="coh", bandwidth=BW, **kw)
        with pytest.raises(SPYValueError, match="does not fit"):
            spy.connectivityanalysis(obj, method="psi", bandwidth=52, **kw)          # h = 26: 52 > 50
    with pytest.raises(SPYValueError, match="equidistant"):
        spy.connectivityanalysis(coupled, method="psi", tapsmofrq=10, foi=[10, 11, 12, 14, 20], bandwidth=2)
    real = spy.SpectralData(np.abs(np.asarray(spectra.data)), samplerate=1000.0, trialdefinition=spectra.trialdefinition)
    with pytest.raises(SPYValueError, match="complex valued spectra"):
        spy.connectivityanalysis(real, method="psi")


def test_jackknife(be, coupled, square):
    """jackknife=True (CrossSpectra.jackknife_hip, one K13 launch per replicate) against the jackknife model on the kept
    single-trial cross spectra.  parity.jackknife_tolerances takes the per-replicate error eps = ulps 2^-24 max|est|; here
    eps = 8 * 2^-24 * 2h - each of the 2h edge products is bounded by 1 and carries the coherency's rounding at unit scale -
    which is passed as an `est` whose maximum is 2h.  The estimate itself is held to the parity criterion plus that eps."""
    T = 5
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = spy.connectivityanalysis(coupled, method="psi", bandwidth=BW, jackknife=True, **KW, **SAME)
    assert not [w for w in rec if "Jackknife is not available" in str(w.message)]
    assert np.array_equal(np.asarray(got.data), np.asarray(square[0].data), equal_nan=True)
    with be.csd_phase_exact(True):
        single = np.asarray(spy.connectivityanalysis(coupled, method="csd", keeptrials=True, **KW, **SAME).data)
    assert single.shape == (T, NF, 33, 33)
    direct, bias, var = PO.jackknife_model(single, H)
    jv, jb = np.asarray(got.jack_var), np.asarray(got.jack_bias)
    assert jv.dtype == np.float32 and jb.dtype == np.float32 and jv.shape == jb.shape == (1, NF, 33, 33)
    outside = np.r_[0:H, NF - H:NF]
    assert np.isnan(jv[0, outside]).all() and np.isnan(jb[0, outside]).all() and np.isnan(got.data[0, outside]).all()
    assert np.isfinite(jv[0, VALID]).all() and np.isfinite(jb[0, VALID]).all()
    d, b, v = direct[VALID], bias[VALID], var[VALID]
    eps = 8 * 2.0 ** -24 * 2 * H
    tol_var, tol_bias = jackknife_tolerances(np.full(1, 2.0 * H), v, T)
    ee = (np.abs(got.data[0, VALID] - d) / (RTOL * np.abs(d) + ATOL_REL * np.abs(d).max() + eps)).max()
    ev = (np.abs(jv[0, VALID].astype(np.float64) - v) / tol_var).max()
    eb = (np.abs(jb[0, VALID].astype(np.float64) - b) / (RTOL * np.abs(b) + tol_bias)).max()
    print(f"jackknife: err/tol estimate {ee:.3g} var {ev:.3g} bias {eb:.3g}")
    assert ee <= 1.0 and ev <= 1.0 and eb <= 1.0, (ee, ev, eb)
    # Nolte's normalisation (five trials make a noisy standard deviation: no threshold is attached)
    z = got.data[0, VALID, 0, 3] / np.sqrt(jv[0, VALID, 0, 3])
    print("psi / sqrt(jack_var) of (0, 3): min %.3g median %.3g" % (z.min(), np.median(z)))
    assert np.all(z > 0)


def test_jackknife_from_spectral_data(be, spectra):
    """SpectralData has no streaming jackknife: the leave-one-out averages are formed on the host and go through the same
    AV class, one replicate per launch; the jackknife arrays follow `channelcmb`.  Tolerances as in test_jackknife."""
    T = 5
    got = spy.connectivityanalysis(spectra, method="psi", bandwidth=BW, jackknife=True)
    with be.csd_phase_exact(True):
        single = np.asarray(spy.connectivityanalysis(spectra, method="csd", keeptrials=True).data)
    direct, bias, var = PO.jackknife_model(single, H)
    jv, jb = np.asarray(got.jack_var), np.asarray(got.jack_bias)
    assert jv.dtype == np.float32 and jb.dtype == np.float32 and jv.shape == jb.shape == (1, NF, 33, 33)
    outside = np.r_[0:H, NF - H:NF]
    assert np.isnan(jv[0, outside]).all() and np.isnan(jb[0, outside]).all()
    d, b, v = direct[VALID], bias[VALID], var[VALID]
    eps = 8 * 2.0 ** -24 * 2 * H
    tol_var, tol_bias = jackknife_tolerances(np.full(1, 2.0 * H), v, T)
    ee = (np.abs(got.data[0, VALID] - d) / (RTOL * np.abs(d) + ATOL_REL * np.abs(d).max() + eps)).max()
    ev = (np.abs(jv[0, VALID].astype(np.float64) - v) / tol_var).max()
    eb = (np.abs(jb[0, VALID].astype(np.float64) - b) / (RTOL * np.abs(b) + tol_bias)).max()
    print(f"jackknife from SpectralData: err/tol estimate {ee:.3g} var {ev:.3g} bias {eb:.3g}")
    assert ee <= 1.0 and ev <= 1.0 and eb <= 1.0, (ee, ev, eb)
    cmb = spy.connectivityanalysis(spectra, method="psi", bandwidth=BW, jackknife=True, channelcmb=[[0, 1], [3, 7]])
    for name in ("jack_var", "jack_bias"):
        assert np.array_equal(np.asarray(getattr(cmb, name)), np.asarray(getattr(got, name))[..., [0, 1], :][..., [3, 7]],
                              equal_nan=True), name


def test_from_time_resolved_spectra(be):
    """complex spectra with 2 time samples per trial: one result per time sample"""
    ntr, L, K, F, Cn = 5, 2, 2, 9, 6
    x = np.stack([PO.spectra(Cn, F, seed=70 + ti, nrep=ntr * K).reshape(ntr, K, F, Cn) for ti in range(L)], axis=1)
    s = spy.SpectralData(x.astype(np.complex64).reshape(ntr * L, K, F, Cn), samplerate=10.0,
                         trialdefinition=[[L * k, L * (k + 1), 0] for k in range(ntr)])
    s.freq, s.taper, s.channel = np.arange(F) * 10.0, np.array([f"t{k}" for k in range(K)]), np.array([f"c{i}" for i in range(Cn)])
    res = spy.connectivityanalysis(s, method="psi", bandwidth=20)
    assert res.data.shape == (L, F, Cn, Cn) and res.cfg["connectivityanalysis"]["h"] == 1
    with be.csd_phase_exact(True):
        coh = np.asarray(spy.connectivityanalysis(s, method="coh", output="complex").data)
    for ti in range(L):
        PO.check(np.asarray(res.data[ti]), coh[ti], 1, what=f"front end, time sample {ti}")


def test_torch_free_host(coupled):
    """abi.Device.phase_slope (NumPy + ctypes over the same entry points) against the model on the complex coherence the
    same device hands out"""
    from syncopy_amd import abi
    from syncopy_amd.specest.tapers import spec_scale, taper_table
    x, si = np.asarray(coupled.data), coupled.sampleinfo
    N = 1000
    tapers = taper_table("dpss", N, N, {"NW": 3.0, "Kmax": 5})
    scale = spec_scale(N, N)
    dev = abi.Device(0)
    try:
        q = dev.upload_trials(x, si)
        coh = dev.coherence(q, tapers, scale, N, detrend=0, output="complex")
        assert coh.shape == (501, 33, 33) and coh.dtype == np.complex64
        for half in (H, 0):
            got = dev.phase_slope(q, tapers, scale, N, detrend=0, half=half)
            PO.check(got, coh, half, what=f"torch-free host, half {half}")
        q.free()
    finally:
        dev.close()
