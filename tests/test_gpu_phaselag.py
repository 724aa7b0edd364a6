"""The phase-lag family on the device: K10 (phaselag_accum_kernel with phaselag_accumulate_csd / phaselag_finalize) and
plv_finalize at the kernel shapes of tests/phaselag_oracle.py against its float64 model under its bounds, and
`spy.connectivityanalysis(method="plv" | "pli" | "wpli" | "wpli_debiased")` from AnalogData and SpectralData against the
model applied to the oracle routines' own tapered spectra.  Every comparison prints its err/tol (pytest -s)."""
import numpy as np
import pytest

import phaselag_oracle as PO
import syncopy_amd as spy
from oracle_routines import ORACLE_CONN, ORACLE_FREQ

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAG = ("pli", "wpli", "wpli_debiased")


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _device_measures(be, spec, split):
    """all four measures of spec (T, K, F, C) through the kernels, the trials in launches of `split`"""
    T, K, F, Cn = spec.shape
    s = _dev(spec)
    acc = torch.zeros((F, Cn, Cn, 4), dtype=torch.float32, device="cuda")
    U = torch.zeros((F, Cn, Cn), dtype=torch.complex64, device="cuda")
    t0 = 0
    for n in split:
        part = s[t0:t0 + n].reshape(-1, F, Cn).contiguous()
        be.phaselag_accumulate(part, K, acc)
        be.ppc_accumulate(part, K, U)
        t0 += n
    assert t0 == T
    got = {m: be.phaselag_finalize(acc, T, True, m).cpu().numpy() for m in LAG}
    got["plv"] = be.plv_finalize(U, T, True).cpu().numpy()
    return got, acc.cpu().numpy()


@pytest.fixture(scope="module")
def models():
    """spectra and model quantities per kernel shape, computed once"""
    out = {}
    for shape in PO.SHAPES:
        spec = PO.spectra(*shape)
        out[shape] = (spec,) + PO.cross_spectra(spec)
    return out


@pytest.mark.parametrize("split", [False, True], ids=["one launch", "two launches"])
@pytest.mark.parametrize("shape", PO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernels_at_dispatch_edges(be, models, shape, split):
    Cn, F, T, K = shape
    spec, S, M = models[shape]
    got, acc = _device_measures(be, spec, [1, T - 1] if split else [T])
    which = [m for m in PO.MEASURES if m != "wpli_debiased" or T >= 3]
    PO.check(got, S, M, K, which=which, what="device " + "-".join(map(str, shape)) + (" split" if split else ""))
    assert np.allclose(got["plv"][:, np.arange(Cn), np.arange(Cn)], 1, atol=1e-6)
    nt = (Cn + 31) // 32
    for bi in range(nt):                      # only the lower triangle at tile granularity is maintained
        for bj in range(bi + 1, nt):
            assert not acc[:, 32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32].any()


@pytest.mark.parametrize("n", [255, 256, 257])
def test_accumulate_csd_block_edges(be, n):
    """one block short, full, and one thread into the second; five trials in launches of 2 + 3"""
    rng = np.random.default_rng(n)
    csd = (rng.normal(size=(5, n)) + 1j * rng.normal(size=(5, n))).astype(np.complex64)
    csd[:, 3] = 0
    csd[2, 7] = 4.0                                                   # an imaginary part of exactly 0 in one trial
    c = _dev(csd)
    acc = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    acc[n] = 7.0
    be.phaselag_accumulate_csd(c[:2].contiguous(), acc[:n])
    be.phaselag_accumulate_csd(c[2:].contiguous(), acc[:n])
    host = acc.cpu().numpy()
    S = csd.reshape(5, 1, 1, n)
    A, B, Q, N, _ = PO.sums(S)
    assert np.all(host[n] == 7.0) and np.array_equal(host[:n, 3], N.ravel()) and np.all(host[3] == 0)
    for k, want in enumerate((A, B, Q)):
        assert np.allclose(host[:n, k], want.ravel(), rtol=8 * PO.U32, atol=8 * PO.U32 * B.max())
    sums = acc[:n].reshape(1, 1, n, 4).contiguous()
    got = {m: be.phaselag_finalize(sums, 5, False, m).cpu().numpy() for m in LAG}
    PO.check(got, S, square=False, which=LAG, what=f"device csd {n}")


def test_finalize_rectangle_and_mirror(be):
    S = PO.cross_spectra(PO.spectra(5, 3, 6, 2, seed=3))[0]
    rect = np.ascontiguousarray(S[:, :, :3, :].astype(np.complex64))           # (T, 3, 3, 5)
    acc = torch.zeros((3, 3, 5, 4), dtype=torch.float32, device="cuda")
    be.phaselag_accumulate_csd(_dev(rect), acc)
    got = {m: be.phaselag_finalize(acc, 6, False, m).cpu().numpy() for m in LAG}
    PO.check(got, rect, square=False, which=LAG, what="device rectangle (3, 3, 5)")
    # lower_only: the upper triangle is never read, the diagonal is exactly 0 whatever the accumulator holds
    full = np.ascontiguousarray(S.astype(np.complex64))
    sq = torch.zeros((3, 5, 5, 4), dtype=torch.float32, device="cuda")
    be.phaselag_accumulate_csd(_dev(full), sq)
    want = {m: be.phaselag_finalize(sq, 6, True, m).cpu().numpy() for m in LAG}
    upper = torch.triu(torch.ones((5, 5), dtype=torch.bool, device="cuda"), 1)
    sq[:, upper] = float("nan")
    sq[:, torch.arange(5), torch.arange(5)] = torch.tensor([1e-9, 1e-9, 0.0, 1.0], device="cuda")
    for m, w in want.items():
        g = be.phaselag_finalize(sq, 6, True, m).cpu().numpy()
        assert np.array_equal(g, w) and np.array_equal(g, g.transpose(0, 2, 1)), m
        assert np.all(g[:, np.arange(5), np.arange(5)] == 0), m
    PO.check(want, full, which=LAG, what="device lower_only (3, 5, 5)")
    with pytest.raises(be.SpyHipError):                            # a lower-triangle accumulator is square
        be.phaselag_finalize(acc, 6, True, "wpli")
    with pytest.raises(be.SpyHipError):                            # a pair of trials at least
        be.phaselag_finalize(acc, 1, False, "wpli")


def test_plv_finalize_against_k7(be):
    """|U| / T from K7's accumulator: on a rectangle element by element, on the lower triangle mirrored"""
    T = 7
    rng = np.random.default_rng(335)
    U = (rng.normal(size=(3, 3, 5)) + 1j * rng.normal(size=(3, 3, 5))).astype(np.complex64) * np.float32(2.0)
    got = be.plv_finalize(_dev(U), T, lower_only=False).cpu().numpy()
    assert np.allclose(got, np.abs(U.astype(np.complex128)) / T, rtol=2 * PO.U32, atol=0)
    spec = PO.spectra(37, 2, 4, 2)
    acc = torch.zeros((2, 37, 37), dtype=torch.complex64, device="cuda")
    be.ppc_accumulate(_dev(spec).reshape(-1, 2, 37), 2, acc)
    plv = be.plv_finalize(acc, 4, lower_only=True).cpu().numpy()
    ppc = be.ppc_finalize(acc, 4, lower_only=True).cpu().numpy()
    # the two finalizers of one accumulator: ppc = (|U|^2 - T) / (T (T - 1))
    assert np.allclose((4.0 * plv.astype(np.float64)) ** 2, ppc.astype(np.float64) * 12 + 4, rtol=1e-5, atol=1e-5)
    PO.check({"plv": plv}, PO.cross_spectra(spec)[0], which=("plv",), what="plv of K7's accumulator")
    with pytest.raises(be.SpyHipError):
        be.plv_finalize(acc, 1, lower_only=True)


def test_too_many_tapers_are_refused(be):
    """161 tapers are 164 864 B of staging, more than any LDS limit the context can hold: K7's refusal, sums untouched"""
    rng = np.random.default_rng(161)
    spec = _dev((rng.normal(size=(161, 1, 3)) + 1j * rng.normal(size=(161, 1, 3))).astype(np.complex64))
    acc0 = rng.normal(size=(1, 3, 3, 4)).astype(np.float32)
    acc = _dev(acc0)
    with pytest.raises(be.SpyHipError, match="code -3"):
        be.phaselag_accumulate(spec, 161, acc)
    assert np.array_equal(acc.cpu().numpy(), acc0)


# ---- the front end ----------------------------------------------------------------------------------------------------------------
TAPERS = dict(tapsmofrq=3, polyremoval=0)


@pytest.fixture(scope="module")
def recording():
    """12 channels x 400 samples x 6 trials at 200 Hz: white noise, every channel with its own share and delay of a
    common source; the spectra of the oracle routines (T, K, F, C) and the model quantities of every pair"""
    rng = np.random.default_rng(12400)
    ntr, n, Cn = 6, 400, 12
    common = rng.normal(size=ntr * n + 8)
    x = rng.normal(size=(ntr * n, Cn))
    for c in range(Cn):
        x[:, c] += (0.3 + 0.1 * c) * common[c % 5:c % 5 + ntr * n]
    trl = np.stack([np.arange(ntr) * n, np.arange(1, ntr + 1) * n, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=200.0, trialdefinition=trl)
    spec = spy.freqanalysis(data, method="mtmfft", output="fourier", keeptapers=True, keeptrials=True,
                            compute_method="sequential", routine_classes=ORACLE_FREQ, **TAPERS)
    x = np.asarray(spec.data)
    assert x.shape[0] == ntr and x.shape[2:] == (n // 2 + 1, Cn) and x.dtype == np.complex64
    return data, spec, x.shape[1], PO.cross_spectra(x)


@pytest.mark.parametrize("method", PO.MEASURES)
def test_from_analog_data(recording, method):
    data, _, K, (S, M) = recording
    res = spy.connectivityanalysis(data, method=method, precision="reference", **TAPERS)
    assert isinstance(res, spy.CrossSpectralData) and res.data.dtype == np.float32 and res.data.shape == (1,) + S.shape[1:]
    assert res.cfg["connectivityanalysis"]["method"] == method and list(res.channel_i) == list(data.channel)
    PO.check({method: res.data[0]}, S, M, K, which=(method,), what="front end, AnalogData")
    again = spy.connectivityanalysis(data, method=method, precision="reference", **TAPERS)
    assert np.array_equal(again.data, res.data)                      # two identical calls: identical bits


@pytest.mark.parametrize("method", PO.MEASURES)
def test_from_mtmfft_spectra(recording, method):
    _, spec, K, (S, M) = recording
    res = spy.connectivityanalysis(spec, method=method)
    assert res.data.shape == (1,) + S.shape[1:] and res.data.dtype == np.float32
    PO.check({method: res.data[0]}, S, M, K, which=(method,), what="front end, mtmfft SpectralData")
    # the per-trial engine path: the oracle's kept single-trial cross spectra into the library's default routine
    seq = spy.connectivityanalysis(spec, method=method, compute_method="sequential", routine_classes=ORACLE_CONN)
    assert seq.data.shape == res.data.shape and seq.data.dtype == np.float32
    PO.check({method: seq.data[0]}, S, M, K, which=(method,), what="sequential path", mirrored=False)
    assert np.array_equal(seq.freq, res.freq) and list(seq.channel_i) == list(res.channel_i)


@pytest.mark.parametrize("method", PO.MEASURES)
def test_channelcmb(recording, method):
    _, spec, K, (S, M) = recording
    names = [str(c) for c in spec.channel]
    send, rec = [names[7], names[2]], [names[2], names[11], names[7], names[0]]
    si, ri = [7, 2], [2, 11, 7, 0]
    res = spy.connectivityanalysis(spec, method=method, channelcmb=[send, rec])
    assert res.data.shape == (1, S.shape[1], 2, 4) and list(res.channel_i) == send and list(res.channel_j) == rec
    cut = lambda a: a[..., si, :][..., ri]                           # noqa: E731
    want = cut(PO.measures(S)[method])
    if method == "plv":
        assert np.allclose(res.data[0], want, rtol=1e-4, atol=2e-5)
        return
    # the zero diagonal stays where sender equals receiver
    assert not res.data[0, :, 0, 2].any() and not res.data[0, :, 1, 0].any()
    b = PO.bounds(cut(S), cut(M), K)
    pairs = np.ones((2, 4), dtype=bool)
    pairs[0, 2] = pairs[1, 0] = False
    ok = (b[method] <= PO.BOUND_CAP) & pairs                         # (the real bins, 0 Hz and Nyquist, are ill-conditioned)
    assert ok[:, pairs].mean() >= 1 - PO.ILL_SHARE
    assert np.all(np.abs(res.data[0] - want)[ok] <= b[method][ok])


@pytest.mark.parametrize("method", PO.MEASURES)
def test_from_time_resolved_spectra(method):
    """mtmconvol spectra with 3 time samples per trial: one result per time sample"""
    rng = np.random.default_rng(3)
    ntr, n, Cn = 6, 400, 5
    x = rng.normal(size=(ntr * n, Cn))
    x[:, 1:] += 0.6 * np.roll(x[:, :1], 1, axis=0)
    trl = np.stack([np.arange(ntr) * n, np.arange(1, ntr + 1) * n, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=200.0, trialdefinition=trl)
    spec = spy.freqanalysis(data, method="mtmconvol", t_ftimwin=0.4, toi=np.array([0.5, 1.0, 1.5]), foilim=[20, 60], tapsmofrq=6,
                            output="fourier", keeptapers=True, compute_method="sequential", routine_classes=ORACLE_FREQ)
    x = np.asarray(spec.data)
    assert x.shape[0] == ntr * 3
    K = x.shape[1]
    x = x.reshape((ntr, 3) + x.shape[1:])
    res = spy.connectivityanalysis(spec, method=method)
    assert res.data.shape == (3, x.shape[3], Cn, Cn) and res.trialdefinition.shape == (1, 3)
    for ti in range(3):
        S, M = PO.cross_spectra(x[:, ti])
        PO.check({method: res.data[ti]}, S, M, K, which=(method,), what=f"front end, time sample {ti}")
    spec.trialdefinition = np.array([[0, 5, 0], [5, 12, 0], [12, 18, 0]])
    with pytest.raises((spy.shared.errors.SPYValueError, NotImplementedError)):      # ragged trials: refused as for ppc
        spy.connectivityanalysis(spec, method=method)


def test_torch_free_host(recording):
    """abi.Device.phase_measure (NumPy + ctypes over the same entry points) against the model on the spectra the same
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
        S, M = PO.cross_spectra(spec)
        got = {m: dev.phase_measure(q, tapers, scale, N, detrend=0, method=m) for m in PO.MEASURES}
        PO.check(got, S, M, 5, what="torch-free host")
        ppc = dev.phase_measure(q, tapers, scale, N, detrend=0, method="ppc")
        assert np.allclose((6.0 * got["plv"].astype(np.float64)) ** 2, ppc.astype(np.float64) * 30 + 6, rtol=1e-5, atol=1e-4)
        with pytest.raises(ValueError):
            dev.phase_measure(q, tapers, scale, N, method="coh")
        q.free()
    finally:
        dev.close()
