"""The envelope correlations on the device: K12 (envcorr_accum_kernel, envcorr_finalize_kernel) at the kernel shapes of
tests/envcorr_oracle.py against its float64 model under its bounds, and
`spy.connectivityanalysis(method="amplcorr" | "powcorr" | "powcorr_ortho")` from AnalogData and SpectralData against the
model applied to the oracle routines' own tapered spectra.  Every comparison prints its err/tol (pytest -s)."""
import numpy as np
import pytest

import envcorr_oracle as EO
import syncopy_amd as spy
from oracle_routines import ORACLE_CONN, ORACLE_FREQ
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


def _device_measure(be, spec, measure, split):
    """`measure` of spec (T, K, F, C) through the kernels, the trials in launches of `split`"""
    T, K, F, Cn = spec.shape
    s = _dev(spec)
    (pair, chan), accumulate, finalize = be.envelope_accumulator(measure, (F, Cn), "cuda")
    t0 = 0
    for n in split:
        accumulate(s[t0:t0 + n].reshape(-1, F, Cn).contiguous(), K, pair, chan)
        t0 += n
    assert t0 == T
    return finalize(pair, chan, T * K).cpu().numpy(), pair.cpu().numpy(), chan.cpu().numpy()


@pytest.fixture(scope="module")
def models():
    """spectra and the three models per kernel shape, computed once"""
    out = {}
    for shape in EO.SHAPES:
        spec = EO.spectra(*shape)
        out[shape] = spec, {m: EO.model(spec, m) for m in EO.MEASURES}
    return out


@pytest.mark.parametrize("split", [False, True], ids=["one launch", "two launches"])
@pytest.mark.parametrize("shape", EO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernels_at_dispatch_edges(be, models, shape, split):
    Cn, F, T, K = shape
    spec, mods = models[shape]
    nt = (Cn + 31) // 32
    got = {}
    for m in EO.MEASURES:
        got[m], pair, chan = _device_measure(be, spec, m, [1, T - 1] if split else [T])
        assert pair.shape == (EO.PLANES[m], F, Cn, Cn) and chan.shape == (F, Cn, 2)
        for bi in range(nt):                      # only the lower triangle at tile granularity is maintained
            for bj in range(bi + 1, nt):
                assert not pair[:, :, 32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32].any()
        assert not chan[:, Cn - 1].any() and np.all(chan[:, :Cn - 1, 0] > 0)
        # the dead and the constant channel: exact zeros, their diagonal included
        assert not got[m][:, Cn - 2:, :].any() and not got[m][:, :, Cn - 2:].any(), m
    EO.check(got, spec, what="device " + "-".join(map(str, shape)) + (" split" if split else ""), models=mods)


def test_finalize_reads_the_lower_triangle_only(be):
    spec = EO.spectra(33, 3, 4, 1)
    for m in EO.MEASURES:
        (pair, chan), accumulate, finalize = be.envelope_accumulator(m, (3, 33), "cuda")
        accumulate(_dev(spec).reshape(-1, 3, 33), 1, pair, chan)
        want = finalize(pair, chan, 4).cpu().numpy()
        pair[:, :, torch.triu(torch.ones((33, 33), dtype=torch.bool, device="cuda"), 1)] = float("nan")
        if m == "powcorr_ortho":
            pair[:, :, torch.arange(33), torch.arange(33)] = 1e-9              # a rounding residue on the diagonal
        assert np.array_equal(finalize(pair, chan, 4).cpu().numpy(), want), m
        with pytest.raises(be.SpyHipError):                        # a pair of repetitions at least
            finalize(pair, chan, 1)
    with pytest.raises(ValueError):
        be.envelope_accumulator("coh", (3, 33), "cuda")


def test_entries_are_in_the_library(be):
    from syncopy_amd import _lib
    for fn in ("spyhip_envcorr_accumulate", "spyhip_envcorr_finalize"):
        assert fn in _lib.SIGNATURES and hasattr(_lib.load(), fn)
    assert be.ENVCORR_MEASURE == EO.MEASURE_CODE and be.ENVCORR_PLANES == EO.PLANES


@pytest.mark.parametrize("measure, ntaper", [("amplcorr", 161), ("powcorr_ortho", 81)])
def test_too_many_tapers_are_refused(be, measure, ntaper):
    """161 tapers are 164 864 B of staging for amplcorr and powcorr, 81 tapers 165 888 B for powcorr_ortho: more than any
    LDS limit the context can hold.  K7's refusal, sums untouched"""
    rng = np.random.default_rng(ntaper)
    spec = _dev((rng.normal(size=(ntaper, 1, 3)) + 1j * rng.normal(size=(ntaper, 1, 3))).astype(np.complex64))
    pair0, chan0 = rng.normal(size=(EO.PLANES[measure], 1, 3, 3)), rng.normal(size=(1, 3, 2))
    pair, chan = _dev(pair0), _dev(chan0)
    with pytest.raises(be.SpyHipError, match="code -3"):
        be.envcorr_accumulate(spec, ntaper, pair, chan, measure)
    assert np.array_equal(pair.cpu().numpy(), pair0) and np.array_equal(chan.cpu().numpy(), chan0)


# ---- the front end ----------------------------------------------------------------------------------------------------------------
TAPERS = dict(tapsmofrq=3, polyremoval=0)    # 11 tapers
INSIDE = dict(foilim=[0.5, 99.5])            # strictly inside (0, Nyquist): the spectra of the two real bins have s = 0


@pytest.fixture(scope="module")
def recording():
    """12 channels x 400 samples x 6 trials at 200 Hz, 11 tapers: white noise under a gain per trial, every channel with its
    own share and delay of a common source; the spectra of the oracle routines (T, K, F, C) and the models on them, on the
    whole frequency axis"""
    rng = np.random.default_rng(12400)
    ntr, n, Cn = 6, 400, 12
    common = rng.normal(size=ntr * n + 8)
    x = rng.normal(size=(ntr * n, Cn))
    for c in range(Cn):
        x[:, c] += (0.3 + 0.1 * c) * common[c % 5:c % 5 + ntr * n]
    x *= np.repeat(np.exp(0.5 * rng.normal(size=ntr)), n)[:, None]
    trl = np.stack([np.arange(ntr) * n, np.arange(1, ntr + 1) * n, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=200.0, trialdefinition=trl)
    spec = spy.freqanalysis(data, method="mtmfft", output="fourier", keeptapers=True, keeptrials=True,
                            compute_method="sequential", routine_classes=ORACLE_FREQ, **TAPERS)
    x = np.asarray(spec.data)
    assert x.shape == (ntr, 11, n // 2 + 1, Cn) and x.dtype == np.complex64
    return data, spec, x, {m: EO.model(x, m) for m in EO.MEASURES}


def _inside(mod):
    """the model of the whole axis cut to the frequencies strictly inside (0, Nyquist)"""
    return {k: v[1:-1] for k, v in mod.items()}


@pytest.mark.parametrize("method", EO.MEASURES)
def test_from_analog_data(recording, method):
    data, _, x, mods = recording
    res = spy.connectivityanalysis(data, method=method, precision="reference", output="angle", **TAPERS, **INSIDE)   # `output` is not used
    assert isinstance(res, spy.CrossSpectralData) and res.data.dtype == np.float32
    assert res.data.shape == (1, x.shape[2] - 2, 12, 12) and res.freq[0] == 0.5 and res.freq[-1] == 99.5
    assert res.cfg["connectivityanalysis"]["method"] == method and list(res.channel_i) == list(data.channel)
    EO.check({method: res.data[0]}, x[:, :, 1:-1], which=(method,), what="front end, AnalogData", models={method: _inside(mods[method])})
    again = spy.connectivityanalysis(data, method=method, precision="reference", **TAPERS, **INSIDE)
    assert np.array_equal(again.data, res.data)                      # two identical calls: identical bits
    # the whole axis, precision="auto": the two real bins are held to finiteness, range, symmetry and diagonal only
    whole = spy.connectivityanalysis(data, method=method, **TAPERS)
    assert whole.data.shape == (1,) + x.shape[2:] + (12,)
    EO.check({method: whole.data[0]}, x, which=(method,), what="front end, whole axis", real_bins=(0, x.shape[2] - 1),
             models={method: mods[method]})


@pytest.mark.parametrize("method", EO.MEASURES)
def test_from_spectral_data_and_channelcmb(recording, method):
    _, spec, x, mods = recording
    res = spy.connectivityanalysis(spec, method=method)
    assert res.data.shape == (1,) + x.shape[2:] + (12,) and res.data.dtype == np.float32
    EO.check({method: res.data[0]}, x, which=(method,), what="front end, SpectralData with kept tapers",
             real_bins=(0, x.shape[2] - 1), models={method: mods[method]})
    # channelcmb: the rectangle is cut from the square of the channels that occur; (7, 7) and (2, 2) keep their diagonal values
    names = [str(c) for c in spec.channel]
    si, ri = [7, 2], [2, 11, 7, 0]
    send, rec = [names[k] for k in si], [names[k] for k in ri]
    cmb = spy.connectivityanalysis(spec, method=method, channelcmb=[send, rec])
    assert cmb.data.shape == (1, x.shape[2], 2, 4) and list(cmb.channel_i) == send and list(cmb.channel_j) == rec
    diag = 0.0 if method == "powcorr_ortho" else 1.0
    assert np.all(cmb.data[0, :, 0, 2] == diag) and np.all(cmb.data[0, :, 1, 0] == diag)
    cut = lambda a: a[1:-1, si, :][:, :, ri]                         # noqa: E731  (the bound does not cover the two real bins)
    want, tol, defined = (cut(mods[method][k]) for k in ("want", "tol", "defined"))
    pairs = np.ones((2, 4), dtype=bool)
    pairs[0, 2] = pairs[1, 0] = False
    assert defined[:, pairs].all() and np.all(tol[:, pairs] <= EO.BOUND_CAP)
    assert np.all(np.abs(cmb.data[0, 1:-1] - want)[:, pairs] <= tol[:, pairs])
    assert np.all(np.isfinite(cmb.data)) and np.all(np.abs(cmb.data) <= 1)
    by_index = spy.connectivityanalysis(spec, method=method, channelcmb=[si, ri])
    assert np.array_equal(by_index.data, cmb.data)


@pytest.mark.parametrize("method", EO.MEASURES)
def test_rules_as_for_ppc(recording, method):
    data, spec, _, _ = recording
    with pytest.warns(UserWarning, match="Jackknife is not available for method " + method):
        jack = spy.connectivityanalysis(data, method=method, jackknife=True, **TAPERS, **INSIDE)
    plain = spy.connectivityanalysis(data, method=method, **TAPERS, **INSIDE)
    assert np.array_equal(jack.data, plain.data) and getattr(jack, "jack_var", None) is None
    for obj in (data, spec):
        with pytest.raises(SPYValueError, match="trial averaging needed for method " + method):
            spy.connectivityanalysis(obj, method=method, keeptrials=True)
        with pytest.raises(SPYValueError, match="only one trial"):
            spy.connectivityanalysis(obj, method=method, select={"trials": [2]})
        with pytest.raises(NotImplementedError, match="batched route only"):
            spy.connectivityanalysis(obj, method=method, compute_method="sequential", routine_classes=ORACLE_CONN)
        with pytest.raises(SPYValueError, match="noise weighting exists for the methods"):
            spy.connectivityanalysis(obj, method=method, noise_weighted=True)
    real = spy.SpectralData(np.abs(np.asarray(spec.data)), samplerate=200.0, trialdefinition=spec.trialdefinition)
    with pytest.raises(SPYValueError, match="complex valued spectra"):
        spy.connectivityanalysis(real, method=method)


def test_from_time_resolved_spectra():
    """complex spectra with 3 time samples per trial: one result per time sample; ragged trials are refused as for ppc"""
    ntr, L, K, F, Cn = 5, 3, 2, 4, 6
    x = np.stack([EO.spectra(Cn, F, ntr, K, seed=70 + ti) for ti in range(L)], axis=1)          # (T, L, K, F, C)
    s = spy.SpectralData(x.reshape(ntr * L, K, F, Cn), samplerate=10.0, trialdefinition=[[L * k, L * (k + 1), 0] for k in range(ntr)])
    s.freq, s.taper, s.channel = np.arange(F) * 10.0, np.array([f"t{k}" for k in range(K)]), np.array([f"c{i}" for i in range(Cn)])
    for method in EO.MEASURES:
        res = spy.connectivityanalysis(s, method=method)
        assert res.data.shape == (L, F, Cn, Cn)
        for ti in range(L):
            EO.check({method: res.data[ti]}, x[:, ti], which=(method,), what=f"front end, time sample {ti}")
    s.trialdefinition = np.array([[0, 5, 0], [5, 12, 0], [12, 15, 0]])
    with pytest.raises((SPYValueError, NotImplementedError)):
        spy.connectivityanalysis(s, method="powcorr")


def test_torch_free_host(recording):
    """abi.Device.envelope_measure (NumPy + ctypes over the same entry points) against the model on the spectra the same
    device hands out"""
    from syncopy_amd import abi
    from syncopy_amd.specest.tapers import spec_scale, taper_table
    data = recording[0]
    x, si = np.asarray(data.data), data.sampleinfo
    N = 400
    tapers = taper_table("dpss", N, N, {"NW": 3.0, "Kmax": 5})
    scale = spec_scale(N, N)
    dev = abi.Device(0)
    try:
        q = dev.upload_trials(x, si)
        spec = dev.mtmfft(q, tapers, scale, N, detrend=0, output="fourier", keeptapers=True)
        assert spec.shape == (6, 5, 201, 12) and spec.dtype == np.complex64
        got = {m: dev.envelope_measure(q, tapers, scale, N, detrend=0, method=m) for m in EO.MEASURES}
        EO.check(got, spec, what="torch-free host", real_bins=(0, 200))
        with pytest.raises(ValueError):
            dev.envelope_measure(q, tapers, scale, N, method="coh")
        q.free()
    finally:
        dev.close()
