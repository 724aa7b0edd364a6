"""The directed measures of the Wilson factors (dtf, pdc: syncopy_amd/csrc/directed.hip, directed_kernel.h,
directed_route.h) without a GPU: the library's own launcher and kernels through the CPU emulation
(tests/emu/directed_emu.cpp) against the float64 model of tests/directed_oracle.py, the route header through a host-only
shim, every rule of the front end - which runs on the per-trial engine path with the model as its routine - and the
directionality of the model itself on a coupled AR(2) network."""
import ctypes as C
import functools

import numpy as np
import pytest

import build_emu
import directed_oracle as DO
import syncopy_amd as spy
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError

KIB = 1024


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(None)
def lib():
    return build_emu.emulated_library("directed")


@functools.lru_cache(None)
def ctx(lds_per_block=0):
    c = build_emu.ctx(lib())
    lib().emu_ctx_set_chip(c, 0, lds_per_block)
    return c


@functools.lru_cache(None)
def shim():
    s = build_emu.build_shim("directed_route_shim.cpp", "libspydirectedroute.so")
    s.dr_norm.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.POINTER(C.c_longlong)]
    return s


def route(n, nfreq, lds=160 * KIB):
    out = (C.c_longlong * 8)()
    shim().dr_norm(n, nfreq, lds, out)
    return dict(zip(("ok", "cached", "kc", "strips", "grid", "threads", "lds", "ld"), list(out)))


def norm(M, w=None, axis=0, squared=False, c=None):
    F, n, _ = M.shape
    out = np.full((F, n, n), np.nan, dtype=np.float32)
    assert lib().spyhip_directed_norm(c or ctx(), ptr(M), ptr(w), F, n, axis, int(squared), ptr(out)) == 0
    return out


def check(got, M, w, axis, squared, what):
    """abs err <= 2^-24: the values lie in [0, 1] and the arithmetic is float64, so what is left is the float32 rounding"""
    want = DO.directed_norm(M, w, axis, squared)
    err = np.abs(got.astype(np.float64) - want).max()
    assert np.isfinite(got).all() and err <= DO.U32, (what, err / DO.U32)
    if squared:     # a DTF sums to 1 over the senders of a receiver, a PDC over the receivers of a sender
        total = got.astype(np.float64).sum(axis=1 if axis == 0 else 2)
        alive = DO.directed_norm(M, w, axis, True).sum(axis=1 if axis == 0 else 2) > 0.5
        assert np.abs(total[alive] - 1).max() <= M.shape[1] * DO.U32, what
        assert np.all(total[~alive] == 0), what


# ---- launcher and kernels on the emulator ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_launcher_against_the_model(shape):
    F, n = shape
    M, w = DO.matrices(F, n), DO.weights(n)
    r = route(n, F)
    assert r["ok"] and r["cached"]
    for axis in (0, 1):
        for weights in (None, w):
            for squared in (False, True):
                build_emu.launches(lib())
                got = norm(M, weights, axis, squared)
                assert build_emu.launches(lib())[:, [0, 1, 2, 3, 6]].tolist() == [[r["grid"], 1, 1, 256, r["lds"]]]
                check(got, M, weights, axis, squared, (shape, axis, weights is not None, squared))


@pytest.mark.parametrize("shape", [(3, 5), (2, 65)], ids=lambda s: "-".join(map(str, s)))
def test_zero_row_and_column_give_zero(shape):
    F, n = shape
    M, w = DO.matrices(F, n, seed=1, dead=True), DO.weights(n, seed=1)
    for axis in (0, 1):
        for squared in (False, True):
            got = norm(M, w, axis, squared)
            check(got, M, w, axis, squared, (shape, axis, squared))
            # [f, sender, receiver]: row 1 of M is receiver 1, column 0 is sender 0
            assert np.all(got[:, :, 1] == 0) and np.all(got[:, 0, :] == 0)
            assert np.count_nonzero(got) == F * (n - 1) * (n - 1)


@pytest.mark.parametrize("shape,lds,kc", [((1, 257), 64 * KIB, 64), ((2, 130), 36 * KIB, 64), ((1, 300), 144 * KIB, 256),
                                          ((1, 400), 160 * KIB, 256)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_strips_that_do_not_fit_lds(shape, lds, kc):
    """the strip is worked through in chunks: sums first, then every chunk again through the tile"""
    F, n = shape
    r = route(n, F, lds)
    assert r["ok"] and not r["cached"] and r["kc"] == kc and r["lds"] <= lds // 2
    M, w = DO.matrices(F, n, seed=2), DO.weights(n, seed=2)
    for axis in (0, 1):
        build_emu.launches(lib())
        got = norm(M, w, axis, True, c=ctx(lds))
        assert build_emu.launches(lib())[:, [0, 3, 6]].tolist() == [[r["grid"], 256, r["lds"]]]
        check(got, M, w, axis, True, (shape, axis, "chunked"))
        assert np.array_equal(got, norm(M, w, axis, True))          # the same sums in the same order of the chunks


def test_launcher_refuses():
    L, c = lib(), ctx()
    M = DO.matrices(2, 5)
    out = np.full((2, 5, 5), 9.0, dtype=np.float32)
    m, o = ptr(M), ptr(out)
    build_emu.launches(L)
    assert [L.spyhip_directed_norm(None, m, None, 2, 5, 0, 0, o), L.spyhip_directed_norm(c, None, None, 2, 5, 0, 0, o),
            L.spyhip_directed_norm(c, m, None, 2, 5, 0, 0, None), L.spyhip_directed_norm(c, m, None, 0, 5, 0, 0, o),
            L.spyhip_directed_norm(c, m, None, 2, 0, 0, 0, o), L.spyhip_directed_norm(c, m, None, 2, 5, 2, 0, o),
            L.spyhip_directed_norm(c, m, None, 2, 5, -1, 0, o), L.spyhip_directed_norm(c, m, None, 2, 5, 0, 0, m)] == [-1] * 8
    # 1 KiB of LDS holds no tile of 32 lines
    big = DO.matrices(1, 70)
    assert L.spyhip_directed_norm(ctx(1024), ptr(big), None, 1, 70, 0, 0, ptr(np.empty((1, 70, 70), "f4"))) == -3
    assert not route(70, 1, 1024)["ok"]
    assert len(build_emu.launches(L)) == 0 and np.all(out == 9.0)


# ---- the route ---------------------------------------------------------------------------------------------------------------
def test_route_table():
    s = shim()
    assert [s.dr_const(i) for i in range(4)] == [32, 256, 4, 256]                # DL, DT, DW, DKC
    tile = lambda kc: (32 * (kc | 1) + 32 + 4 * 32) * 8                          # the tile, the sums, the partial sums
    for lds in (160 * KIB, 64 * KIB):
        for n in list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 315, 316, 317, 318, 511, 512, 1000, 4096]:
            for F in (1, 7, 8, 9, 2049):
                r = route(n, F, lds)
                assert r["ok"] and r["threads"] == 256
                assert r["strips"] == (n + 31) // 32 and r["grid"] == r["strips"] * ((F + 7) // 8) * 8
                assert r["ld"] % 2 == 1 and r["ld"] >= r["kc"] and r["lds"] == tile(r["kc"]) <= lds // 2
                if tile(n) <= lds // 2:
                    assert r["cached"] and r["kc"] == n
                else:
                    assert not r["cached"] and r["kc"] == max(k for k in (64, 128, 256) if tile(k) <= lds // 2) < n
                # the kernel's block map: matrix (slot // strips) * 8 + id % 8, strip slot % strips - every strip of every
                # matrix exactly once
                if F <= 9 and n <= 129:
                    seen = sorted(((i >> 3) // r["strips"] * 8 + (i & 7), (i >> 3) % r["strips"]) for i in range(r["grid"]))
                    assert [p for p in seen if p[0] < F] == [(f, t) for f in range(F) for t in range(r["strips"])]
    # whole strips at the 160 KiB of the MI355X up to n = 315, the production shape included
    assert route(315, 1)["cached"] and not route(316, 1)["cached"] and route(256, 2049)["grid"] == 8 * 2056
    # an LDS too small for two workgroups takes one, a small matrix whole
    assert route(70, 1, 24 * KIB) == {**route(70, 1, 24 * KIB), "ok": 1, "cached": 0, "kc": 64}
    assert route(40, 1, 16 * KIB) == {**route(40, 1, 16 * KIB), "ok": 1, "cached": 1, "kc": 40}


# ---- the front end -----------------------------------------------------------------------------------------------------------
def on_model(method, **kw):
    return dict(method=method, compute_method="sequential", routine_classes=DO.oracle_classes(), **kw)


@functools.lru_cache(None)
def network(ntrials=50, nsamples=500, coupling=0.25, seed=42):
    adj = np.zeros((3, 3))
    adj[0, 1] = coupling
    return spy.synthdata.ar2_network(AdjMat=adj, nSamples=nsamples, nTrials=ntrials, seed=seed, samplerate=1000)


def _spectral(ntrials=30, nchan=3, K=2, F=9, seed=1):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(ntrials, K, F, nchan)) + 1j * rng.normal(size=(ntrials, K, F, nchan))).astype(np.complex64)
    x[..., 1] += 0.5 * x[..., 0]
    s = spy.SpectralData(x, samplerate=10.0, trialdefinition=[[k, k + 1, 0] for k in range(ntrials)])
    s.freq, s.taper, s.channel = np.arange(F) * 10.0, np.array([f"t{k}" for k in range(K)]), np.array([f"c{i}" for i in range(nchan)])
    return s


def test_method_names_and_abi():
    from syncopy_amd import _lib, abi, backend
    from syncopy_amd.shared.const_def import connectivityMethods, directedMethods
    assert directedMethods == DO.MEASURES and set(DO.MEASURES) <= set(connectivityMethods)
    assert "spyhip_directed_norm" in _lib.SIGNATURES and "spyhip_zinv" in _lib.SIGNATURES and hasattr(lib(), "spyhip_directed_norm")
    assert all(callable(getattr(mod, fn)) for mod in (backend, abi.Device) for fn in ("zinv", "directed_norm"))
    with pytest.raises(SPYValueError, match="dtf, pdc"):
        spy.connectivityanalysis(network(), method="dtf2")


@pytest.mark.parametrize("method", DO.MEASURES)
def test_result_of_the_front_end(method):
    d = network()
    res = spy.connectivityanalysis(d, tapsmofrq=5, **on_model(method))
    F = 500 // 2 + 1
    assert isinstance(res, spy.CrossSpectralData) and res.data.dtype == np.float32 and res.data.shape == (1, F, 3, 3)
    assert np.array_equal(res.freq, np.fft.rfftfreq(500, 1e-3))
    assert list(res.channel_i) == list(d.channel) == list(res.channel_j)
    assert res.cfg["connectivityanalysis"]["method"] == method
    assert set(res.info) == {"converged", "max rel. err", "reg. factor", "initial cond. num"} and res.info["converged"] is True
    assert np.all((res.data >= 0) & (res.data <= 1)) and np.all(res.data[0][:, np.arange(3), np.arange(3)] > 0.5)   # the diagonal is kept
    pw = spy.connectivityanalysis(d, tapsmofrq=5, output="pow", **on_model(method))
    assert np.allclose(pw.data, res.data.astype(np.float64) ** 2, rtol=1e-6, atol=0)
    assert np.allclose(pw.data[0].sum(axis=1 if method == "dtf" else 2), 1, atol=3 * DO.U32)
    nw = spy.connectivityanalysis(d, tapsmofrq=5, noise_weighted=True, **on_model(method))
    assert nw.data.shape == res.data.shape and not np.array_equal(nw.data, res.data)
    # the trial-averaged CSD of the same call is what the model factorises (granger's ST stage: demeaned tapers)
    H, Sigma, info = DO.chain(_granger_csd(d))
    assert info["converged"]
    for out, kw in ((res, {}), (pw, dict(output="pow")), (nw, dict(noise_weighted=True))):
        assert np.allclose(out.data[0], DO.measure(method, H, Sigma, **kw), rtol=0, atol=DO.U32)
    with pytest.warns(UserWarning, match="Jackknife is not available for method " + method):
        jack = spy.connectivityanalysis(d, tapsmofrq=5, jackknife=True, **on_model(method))
    assert np.array_equal(jack.data, res.data) and getattr(jack, "jack_var", None) is None
    sel = spy.connectivityanalysis(d, tapsmofrq=5, select={"channel": [0, 1]}, **on_model(method))
    assert sel.data.shape == (1, F, 2, 2) and list(sel.channel_i) == list(d.channel[:2])


def _granger_csd(d):
    """the trial-averaged cross spectra of granger's (and the directed methods') ST stage, from the oracle"""
    from oracle_routines import OracleCrossSpectra
    from syncopy_amd.connectivity import connectivity_analysis as ca
    keep = {}

    class Keep(OracleCrossSpectra):
        def compute(self, data, out, **kw):
            super().compute(data, out, **kw)
            keep["csd"], keep["demean"] = np.asarray(out.data)[0], self.cfg["demean_taper"]

    spy.connectivityanalysis(d, tapsmofrq=5, **{**on_model("dtf"), "routine_classes": {**DO.oracle_classes(), "csd": Keep}})
    assert keep["demean"] is True and ca.directedMethods == DO.MEASURES
    return keep["csd"]


@pytest.mark.parametrize("method", DO.MEASURES)
def test_rules_as_for_granger(method, monkeypatch):
    d = network()
    for kw in (dict(foi=[10, 20]), dict(foilim=[10, 100])):
        with pytest.raises(SPYValueError, match="no foi specification"):
            spy.connectivityanalysis(d, **kw, **on_model(method))
    for keep in (True, "yes", 1):
        with pytest.raises(SPYValueError, match="trial averaging needed for method " + method):
            spy.connectivityanalysis(d, keeptrials=keep, **on_model(method))
    for output in ("complex", "angle", "fourier", "real", "imag", "power", None):
        with pytest.raises(SPYValueError, match="'abs' or 'pow'"):
            spy.connectivityanalysis(d, output=output, **on_model(method))
    with pytest.raises(SPYTypeError):
        spy.connectivityanalysis(d, noise_weighted="yes", **on_model(method))
    with pytest.raises(SPYTypeError):
        spy.connectivityanalysis(d, channelcmb=[[0], [1]], **on_model(method))         # channelcmb wants SpectralData
    one = spy.AnalogData(np.zeros((100, 2), "f4"), samplerate=100)
    with pytest.raises(SPYValueError, match="only one trial"):
        spy.connectivityanalysis(one, **on_model(method))
    few = network(ntrials=20)
    with pytest.warns(UserWarning, match="numerically unstable"):                      # 3 channels / 20 trials > 0.1
        spy.connectivityanalysis(few, tapsmofrq=5, **on_model(method))
    # a build without the Wilson kernels registers no routine
    from syncopy_amd.connectivity import AV_compRoutines
    monkeypatch.delattr(AV_compRoutines, "DirectedMeasure")
    classes = {k: v for k, v in DO.oracle_classes().items() if k not in DO.MEASURES}
    with pytest.raises(NotImplementedError, match="not part of this build"):
        spy.connectivityanalysis(d, tapsmofrq=5, method=method, compute_method="sequential", routine_classes=classes)


@pytest.mark.parametrize("method", ["coh", "granger", "csd", "ppc", "wpli", "corr"])
def test_noise_weighted_is_for_the_directed_methods_only(method):
    with pytest.raises(SPYValueError, match="noise_weighted"):
        spy.connectivityanalysis(network(), method=method, noise_weighted=True, compute_method="sequential",
                                 routine_classes=DO.oracle_classes())


@pytest.mark.parametrize("method", DO.MEASURES)
def test_spectral_data_and_channelcmb(method):
    s = _spectral()
    res = spy.connectivityanalysis(s, **on_model(method))
    assert res.data.shape == (1, 9, 3, 3) and res.data.dtype == np.float32 and "converged" in res.info
    x = np.asarray(s.data).astype(np.complex128)                                       # (T, K, F, C)
    csd = (x[..., :, None] * x[..., None, :].conj()).mean(axis=1).mean(axis=0)
    H, Sigma, _ = DO.chain(csd.astype(np.complex64))
    assert np.allclose(res.data[0], DO.measure(method, H, Sigma), rtol=2e-3, atol=2e-4)
    # channelcmb: the multivariate measure, post-selected
    send, rec = ["c2", "c0"], ["c0", "c1", "c2"]
    part = spy.connectivityanalysis(s, channelcmb=[send, rec], **on_model(method))
    assert part.data.shape == (1, 9, 2, 3) and list(part.channel_i) == send and list(part.channel_j) == rec
    assert np.array_equal(part.data, res.data[:, :, [2, 0], :][:, :, :, [0, 1, 2]]) and part.info == res.info
    by_index = spy.connectivityanalysis(s, channelcmb=[[2, 0], [0, 1, 2]], **on_model(method))
    assert np.array_equal(by_index.data, part.data)
    real = spy.SpectralData(np.abs(np.asarray(s.data)), samplerate=10.0, trialdefinition=s.trialdefinition)
    with pytest.raises(SPYValueError, match="complex valued spectra"):
        spy.connectivityanalysis(real, **on_model(method))


# ---- directionality, on the model alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_weighted", [False, True])
@pytest.mark.parametrize("method", DO.MEASURES)
def test_direction_of_the_coupling(method, noise_weighted):
    """One coupling 0 -> 1 among three AR(2) channels (50 trials of 500 samples, coupling 0.25, seed 42): at the AR(2)
    peak the chain model gives 0.75 for 0 -> 1 and 0.045 for 1 -> 0, a ratio of 17 for every measure; >= 3 is asserted.
    The device inherits the property through its parity with this model (tests/test_gpu_directed.py)."""
    d = network()
    res = spy.connectivityanalysis(d, tapsmofrq=5, noise_weighted=noise_weighted, **on_model(method))
    k = int(np.argmin(np.abs(res.freq - spy.synthdata.ar2_peak_freq(0.55, -0.8, 1000))))
    x = res.data[0, k].astype(np.float64)
    assert x[0, 1] >= 3 * x[1, 0] and x[0, 1] >= 3 * max(x[0, 2], x[2, 0], x[1, 2], x[2, 1]) and x[0, 1] > 0.5
