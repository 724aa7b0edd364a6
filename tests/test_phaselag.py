"""The phase-lag family (plv, pli, wpli, wpli_debiased: syncopy_amd/csrc/phaselag.hip, phaselag_kernel.h) without a GPU:
the model's own conventions, the library's launchers and kernels through the CPU emulation (tests/emu/phaselag_emu.cpp)
at the kernel shapes of tests/phaselag_oracle.py under its bounds, every refusal of the launchers, and every rule of the
front end - which runs on the per-trial engine path with the emulated library as its routine."""
import ctypes as C
import functools

import numpy as np
import pytest

import build_emu
import csd_drive as D
import phaselag_oracle as PO
import syncopy_amd as spy
from oracle_routines import ORACLE_CONN
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError

ptr = D.ptr


@functools.lru_cache(None)
def lib():
    return build_emu.emulated_library("phaselag")


@functools.lru_cache(None)
def ctx(lds_per_block=0):
    c = build_emu.ctx(lib())
    lib().emu_ctx_set_chip(c, D.NO_RECUT, lds_per_block)
    return c


def accumulate(spec, acc, split=None):
    """spyhip_phaselag_accumulate on spec (T, K, F, C) complex64, in launches of `split` trials"""
    T, K, F, Cn = spec.shape
    t0 = 0
    for n in split or [T]:
        part = np.ascontiguousarray(spec[t0:t0 + n])
        assert lib().spyhip_phaselag_accumulate(ctx(), ptr(part), n, K, F, Cn, ptr(acc)) == 0
        t0 += n
    assert t0 == T


def accumulate_csd(csd, acc):
    csd = np.ascontiguousarray(csd, dtype=np.complex64)
    assert lib().spyhip_phaselag_accumulate_csd(ctx(), ptr(csd), csd.shape[0], acc.size // 4, ptr(acc)) == 0


def finalize(acc, T, lower_only, measure):
    F, ni, nj, _ = acc.shape
    out = np.full((F, ni, nj), np.nan, dtype=np.float32)
    assert lib().spyhip_phaselag_finalize(ctx(), ptr(acc), F, ni, nj, int(lower_only), T, PO.MEASURE_CODE[measure], ptr(out)) == 0
    return out


def plv_finalize(U, T, lower_only):
    F, ni, nj = U.shape
    out = np.full((F, ni, nj), np.nan, dtype=np.float32)
    assert lib().spyhip_plv_finalize(ctx(), ptr(U), F, ni, nj, int(lower_only), T, ptr(out)) == 0
    return out


def emulated(measure):
    """the library's default routine of the per-trial engine path (AV_compRoutines.phase_lag) on the emulated library:
    kept single-trial cross spectra (T, F, Ni, Nj) -> (1, F, Ni, Nj)"""
    def routine(st_csd):
        st_csd = np.ascontiguousarray(st_csd, dtype=np.complex64)
        T = st_csd.shape[0]
        if measure == "plv":
            U = np.zeros(st_csd.shape[1:], dtype=np.complex64)
            D.ppc_accumulate_csd(st_csd, U)
            return plv_finalize(U, T, False)[np.newaxis]
        acc = np.zeros(st_csd.shape[1:] + (4,), dtype=np.float32)
        accumulate_csd(st_csd, acc)
        return finalize(acc, T, False, measure)[np.newaxis]
    return routine


def on_emulator(method):
    return dict(method=method, compute_method="sequential", routine_classes={**ORACLE_CONN, method: emulated(method)})


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_model_hand_check():
    """T = 2, K = 1, s = (+1, -3)"""
    S = np.array([1j, -3j]).reshape(2, 1, 1, 1)
    m = PO.measures(S, diagonal=False)
    assert m["pli"].item() == 0 and m["wpli"].item() == 0.5 and m["wpli_debiased"].item() == -1.0 and m["plv"].item() == 0
    S = np.array([2 + 1j, 1 + 3j, -1 + 0j]).reshape(3, 1, 1, 1)       # sign(0) = 0
    m = PO.measures(S, diagonal=False)
    assert m["pli"].item() == pytest.approx(2 / 3) and m["wpli"].item() == 1.0
    assert m["wpli_debiased"].item() == pytest.approx((16 - 10) / (16 - 10))
    assert PO.gamma(3) == pytest.approx(3 * 2.0 ** -24, rel=1e-6)


def test_model_conventions():
    spec = PO.spectra(6, 3, 5, 2)
    m = PO.from_spectra(spec)
    i = np.arange(6)
    for name in PO.MEASURES:
        assert np.array_equal(m[name], m[name].transpose(0, 2, 1)), name
    for name in ("pli", "wpli", "wpli_debiased"):
        assert np.all(m[name][:, i, i] == 0), name
        assert np.all(m[name][:, 5, :] == 0) and np.all(m[name][:, :, 5] == 0), name        # the dead channel
        assert np.all(m[name][:, :5, :5][:, ~np.eye(5, dtype=bool)] != 0), name
    assert np.allclose(m["plv"][:, i, i], 1, atol=1e-12) and np.all(m["plv"][:, 5, :] == 1)   # K7's phasor of 0 is 1
    assert np.all((m["pli"] >= 0) & (m["pli"] <= 1)) and np.all((m["wpli"] >= 0) & (m["wpli"] <= 1 + 1e-12))
    # a positive scale (the spectral normalisation 1 / K) changes nothing
    S, _ = PO.cross_spectra(spec)
    for name, v in PO.measures(S / 2).items():
        assert np.allclose(v, m[name], rtol=1e-12, atol=0), name


# ---- launchers and kernels on the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["one launch", "two launches"])
@pytest.mark.parametrize("shape", PO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernels_at_dispatch_edges(shape, split):
    Cn, F, T, K = shape
    spec = PO.spectra(*shape)
    S, M = PO.cross_spectra(spec)
    acc = np.zeros((F, Cn, Cn, 4), dtype=np.float32)
    build_emu.launches(lib())
    accumulate(spec, acc, [1, T - 1] if split else None)
    nt = (Cn + 31) // 32
    log = build_emu.launches(lib())
    assert log[:, [0, 3, 6]].tolist() == [[8 * ((F + 7) // 8) * nt * (nt + 1) // 2, 256, 2 * 2 * K * 32 * 8]] * (2 if split else 1)
    got = {m: finalize(acc, T, True, m) for m in ("pli", "wpli", "wpli_debiased")}
    U = np.zeros((F, Cn, Cn), dtype=np.complex64)
    D.ppc_accumulate(spec.reshape(-1, F, Cn), K, U)
    got["plv"] = plv_finalize(U, T, True)
    which = [m for m in PO.MEASURES if m != "wpli_debiased" or T >= 3]
    PO.check(got, S, M, K, which=which, what="emulator " + "-".join(map(str, shape)))
    assert np.allclose(got["plv"][:, np.arange(Cn), np.arange(Cn)], 1, atol=1e-6)
    # only the lower triangle at tile granularity is maintained
    for bi in range(nt):
        for bj in range(bi + 1, nt):
            assert not acc[:, 32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32].any()


@pytest.mark.parametrize("n", [255, 256, 257])
def test_accumulate_csd_block_edges(n):
    rng = np.random.default_rng(n)
    csd = (rng.normal(size=(5, n)) + 1j * rng.normal(size=(5, n))).astype(np.complex64)
    csd[:, 3] = 0
    csd[2, 7] = 4.0                                                   # an imaginary part of exactly 0 in one trial
    acc = np.zeros((n + 1, 4), dtype=np.float32)
    acc[n] = 7.0
    accumulate_csd(csd[:2], acc[:n])
    accumulate_csd(csd[2:], acc[:n])
    assert np.all(acc[n] == 7.0)
    S = csd.reshape(5, 1, 1, n)
    A, B, Q, N, _ = PO.sums(S)
    assert np.array_equal(acc[:n, 3], N.ravel()) and np.all(acc[3] == 0)
    for k, want in enumerate((A, B, Q)):
        assert np.allclose(acc[:n, k], want.ravel(), rtol=8 * PO.U32, atol=8 * PO.U32 * B.max())
    got = {m: finalize(acc[:n].reshape(1, 1, n, 4), 5, False, m) for m in ("pli", "wpli", "wpli_debiased")}
    PO.check(got, S, square=False, which=("pli", "wpli", "wpli_debiased"), what=f"csd {n}")


def test_finalize_rectangle_and_mirror():
    S = PO.cross_spectra(PO.spectra(5, 3, 6, 2, seed=3))[0]
    rect = np.ascontiguousarray(S[:, :, :3, :].astype(np.complex64))           # (T, 3, 3, 5)
    acc = np.zeros((3, 3, 5, 4), dtype=np.float32)
    accumulate_csd(rect, acc)
    got = {m: finalize(acc, 6, False, m) for m in ("pli", "wpli", "wpli_debiased")}
    U = np.zeros((3, 3, 5), dtype=np.complex64)
    D.ppc_accumulate_csd(rect, U)
    got["plv"] = plv_finalize(U, 6, False)
    PO.check(got, rect, square=False, what="rectangle (3, 3, 5)")
    # element-wise on a rectangle: position (i, i) is whatever its sums give, no diagonal is written
    assert np.all(got["wpli"][:, :, :4][:, ~np.eye(3, 4, dtype=bool)] > 0)
    # lower_only: the upper triangle is never read, the diagonal is exactly 0 whatever the accumulator holds
    full = np.ascontiguousarray(S.astype(np.complex64))
    sq = np.zeros((3, 5, 5, 4), dtype=np.float32)
    accumulate_csd(full, sq)
    want = {m: finalize(sq, 6, True, m) for m in ("pli", "wpli", "wpli_debiased")}
    upper = np.triu(np.ones((5, 5), dtype=bool), 1)
    sq[:, upper] = np.nan
    sq[:, np.arange(5), np.arange(5)] = (1e-9, 1e-9, 0.0, 1.0)                  # a rounding residue on the diagonal
    Uq = np.zeros((3, 5, 5), dtype=np.complex64)
    D.ppc_accumulate_csd(full, Uq)
    plv = plv_finalize(Uq, 6, True)
    Uq[:, upper] = np.nan
    assert np.array_equal(plv_finalize(Uq, 6, True), plv) and np.array_equal(plv, plv.transpose(0, 2, 1))
    for m, w in want.items():
        g = finalize(sq, 6, True, m)
        assert np.array_equal(g, w) and np.array_equal(g, g.transpose(0, 2, 1)), m
        assert np.all(g[:, np.arange(5), np.arange(5)] == 0), m
    PO.check({**want, "plv": plv}, full, what="lower_only (3, 5, 5)")


def test_launchers_refuse():
    L, c = lib(), ctx()
    spec = PO.spectra(5, 3, 2, 2)
    acc = np.zeros((3, 5, 5, 4), dtype=np.float32)
    accumulate(spec, acc)
    keep = acc.copy()
    U = np.ones((3, 5, 5), dtype=np.complex64)
    out = np.full((3, 5, 5), 9.0, dtype=np.float32)
    s, a, u, o = ptr(spec), ptr(acc), ptr(U), ptr(out)
    build_emu.launches(L)
    # null arguments
    assert [L.spyhip_phaselag_accumulate(None, s, 2, 2, 3, 5, a), L.spyhip_phaselag_accumulate(c, None, 2, 2, 3, 5, a),
            L.spyhip_phaselag_accumulate(c, s, 2, 2, 3, 5, None), L.spyhip_phaselag_accumulate_csd(None, s, 2, 75, a),
            L.spyhip_phaselag_accumulate_csd(c, None, 2, 75, a), L.spyhip_phaselag_accumulate_csd(c, s, 2, 75, None),
            L.spyhip_phaselag_finalize(None, a, 3, 5, 5, 1, 2, 1, o), L.spyhip_phaselag_finalize(c, None, 3, 5, 5, 1, 2, 1, o),
            L.spyhip_phaselag_finalize(c, a, 3, 5, 5, 1, 2, 1, None), L.spyhip_plv_finalize(None, u, 3, 5, 5, 1, 2, o),
            L.spyhip_plv_finalize(c, None, 3, 5, 5, 1, 2, o), L.spyhip_plv_finalize(c, u, 3, 5, 5, 1, 2, None)] == [-1] * 12
    # shapes
    assert [L.spyhip_phaselag_accumulate(c, s, -1, 2, 3, 5, a), L.spyhip_phaselag_accumulate(c, s, 2, 0, 3, 5, a),
            L.spyhip_phaselag_accumulate(c, s, 2, 2, 0, 5, a), L.spyhip_phaselag_accumulate(c, s, 2, 2, 3, 0, a),
            L.spyhip_phaselag_accumulate_csd(c, s, -1, 75, a), L.spyhip_phaselag_accumulate_csd(c, s, 2, 0, a),
            L.spyhip_phaselag_finalize(c, a, 0, 5, 5, 1, 2, 1, o), L.spyhip_phaselag_finalize(c, a, 3, 0, 5, 0, 2, 1, o),
            L.spyhip_phaselag_finalize(c, a, 3, 5, 0, 0, 2, 1, o), L.spyhip_plv_finalize(c, u, 0, 5, 5, 1, 2, o),
            L.spyhip_plv_finalize(c, u, 3, 0, 5, 0, 2, o), L.spyhip_plv_finalize(c, u, 3, 5, 0, 0, 2, o)] == [-1] * 12
    # fewer than two trials; lower_only on a rectangle (which the element-wise form accepts); a measure that is none
    assert [L.spyhip_phaselag_finalize(c, a, 3, 5, 5, 1, 1, 1, o), L.spyhip_plv_finalize(c, u, 3, 5, 5, 1, 1, o),
            L.spyhip_phaselag_finalize(c, a, 3, 5, 5, 0, 0, 1, o), L.spyhip_plv_finalize(c, u, 3, 5, 5, 0, 0, o),
            L.spyhip_phaselag_finalize(c, a, 3, 5, 3, 1, 2, 1, o), L.spyhip_plv_finalize(c, u, 3, 5, 3, 1, 2, o),
            L.spyhip_phaselag_finalize(c, a, 3, 5, 5, 1, 2, 3, o), L.spyhip_phaselag_finalize(c, a, 3, 5, 5, 1, 2, -1, o)] == [-1] * 8
    # tapers that do not fit the LDS staging buffer: K7's code.  1 KiB holds the two buffers of one taper
    small = ctx(lds_per_block=1024)
    assert L.spyhip_phaselag_accumulate(small, s, 2, 2, 3, 5, a) == -3
    assert len(build_emu.launches(L)) == 0                                      # nothing ran
    assert np.array_equal(acc, keep) and np.all(out == 9.0)
    one = np.zeros_like(acc)
    assert L.spyhip_phaselag_accumulate(small, s, 4, 1, 3, 5, ptr(one)) == 0 and one.any()
    # no trials: nothing to do
    assert [L.spyhip_phaselag_accumulate(c, s, 0, 2, 3, 5, a), L.spyhip_phaselag_accumulate_csd(c, s, 0, 75, a)] == [0, 0]
    assert len(build_emu.launches(L)) == 1 and np.array_equal(acc, keep)
    assert L.spyhip_phaselag_finalize(c, a, 3, 5, 3, 0, 2, 1, o) == 0 and L.spyhip_plv_finalize(c, u, 3, 5, 3, 0, 2, o) == 0


# ---- the front end ----------------------------------------------------------------------------------------------------------------
def _analog(nchan=4, ntrials=5, nsamples=120, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(ntrials * nsamples, nchan)).astype(np.float32)
    x[:, 1] += 0.7 * np.roll(x[:, 0], 2)
    return spy.AnalogData(x, samplerate=100.0, trialdefinition=[[k * nsamples, (k + 1) * nsamples, 0] for k in range(ntrials)])


def _spectral(lengths, nchan=4, K=2, F=3, seed=1):
    """complex SpectralData with trials of `lengths` time samples"""
    rng = np.random.default_rng(seed)
    n = int(np.sum(lengths))
    x = (rng.normal(size=(n, K, F, nchan)) + 1j * rng.normal(size=(n, K, F, nchan))).astype(np.complex64)
    edges = np.concatenate(([0], np.cumsum(lengths)))
    s = spy.SpectralData(x, samplerate=10.0, trialdefinition=[[a, b, 0] for a, b in zip(edges[:-1], edges[1:])])
    s.freq, s.taper, s.channel = np.arange(F) * 10.0, np.array([f"t{k}" for k in range(K)]), np.array([f"c{i}" for i in range(nchan)])
    return s


def test_method_names():
    from syncopy_amd.shared.const_def import connectivityMethods, phaseMethods
    assert set(PO.MEASURES) <= set(connectivityMethods) and set(phaseMethods) == set(PO.MEASURES) | {"ppc"}
    from syncopy_amd import _lib
    for fn in ("spyhip_phaselag_accumulate", "spyhip_phaselag_accumulate_csd", "spyhip_phaselag_finalize", "spyhip_plv_finalize"):
        assert fn in _lib.SIGNATURES and hasattr(lib(), fn)
    with pytest.raises(SPYValueError, match="wpli_debiased"):
        spy.connectivityanalysis(_analog(), method="wpli2")


@pytest.mark.parametrize("method", PO.MEASURES)
def test_from_analog_data(method):
    d = _analog()
    kw = dict(tapsmofrq=3, foilim=[5, 30])
    S = spy.connectivityanalysis(d, method="csd", keeptrials=True, compute_method="sequential", routine_classes=ORACLE_CONN, **kw)
    res = spy.connectivityanalysis(d, output="angle", **on_emulator(method), **kw)          # `output` is ignored
    assert isinstance(res, spy.CrossSpectralData) and res.data.dtype == np.float32
    assert res.data.shape == (1,) + S.data.shape[1:] and np.array_equal(res.freq, S.freq)
    assert list(res.channel_i) == list(d.channel) == list(res.channel_j)
    assert res.cfg["connectivityanalysis"]["method"] == method
    PO.check({method: res.data[0]}, np.asarray(S.data), which=(method,), what="AnalogData", mirrored=False)
    sel = spy.connectivityanalysis(d, select={"channel": [0, 2], "trials": [0, 1, 3]}, **on_emulator(method), **kw)
    Ssel = np.asarray(S.data)[[0, 1, 3]][..., [0, 2], :][..., [0, 2]]
    PO.check({method: sel.data[0]}, Ssel, which=(method,), what="AnalogData, selection", mirrored=False)


@pytest.mark.parametrize("method", PO.MEASURES)
def test_rules_as_for_ppc(method):
    d = _analog()
    for keep in (True, "yes", 1):
        with pytest.raises(SPYValueError, match="trial averaging needed for method " + method):
            spy.connectivityanalysis(d, keeptrials=keep, **on_emulator(method))
    one = spy.AnalogData(np.zeros((100, 2), "f4"), samplerate=100)
    with pytest.raises(SPYValueError, match="only one trial"):
        spy.connectivityanalysis(one, **on_emulator(method))
    with pytest.raises(SPYValueError, match="only one trial"):
        spy.connectivityanalysis(d, select={"trials": [2]}, **on_emulator(method))
    with pytest.warns(UserWarning, match="Jackknife is not available for method " + method):
        jack = spy.connectivityanalysis(d, jackknife=True, tapsmofrq=3, **on_emulator(method))
    plain = spy.connectivityanalysis(d, tapsmofrq=3, **on_emulator(method))
    assert np.array_equal(jack.data, plain.data) and getattr(jack, "jack_var", None) is None
    with pytest.raises(SPYTypeError):
        spy.connectivityanalysis(d, channelcmb=[[0], [1]], **on_emulator(method))     # channelcmb wants SpectralData


@pytest.mark.parametrize("method", PO.MEASURES)
def test_from_spectral_data(method):
    s = _spectral([1] * 6)
    res = spy.connectivityanalysis(s, **on_emulator(method))
    x = np.asarray(s.data)[:, None]                                                       # (T, K, F, C) per time sample
    S = PO.cross_spectra(x[:, 0])[0].astype(np.complex64)
    assert res.data.shape == (1, 3, 4, 4) and res.data.dtype == np.float32
    PO.check({method: res.data[0]}, S, which=(method,), what="SpectralData", mirrored=False)
    # time-resolved spectra of equal trial lengths: one result per time sample
    s = _spectral([3, 3, 3, 3, 3])
    res = spy.connectivityanalysis(s, **on_emulator(method))
    assert res.data.shape == (3, 3, 4, 4)
    x = np.asarray(s.data).reshape(5, 3, 2, 3, 4)
    for ti in range(3):
        S = PO.cross_spectra(x[:, ti])[0].astype(np.complex64)
        PO.check({method: res.data[ti]}, S, which=(method,), what=f"time sample {ti}", mirrored=False)
    with pytest.raises(SPYValueError, match="trials of equal length"):
        spy.connectivityanalysis(_spectral([3, 2, 3]), **on_emulator(method))
    real = spy.SpectralData(np.abs(np.asarray(s.data)), samplerate=10.0, trialdefinition=s.trialdefinition)
    with pytest.raises(SPYValueError, match="complex valued spectra"):
        spy.connectivityanalysis(real, **on_emulator(method))


@pytest.mark.parametrize("method", PO.MEASURES)
def test_channelcmb(method):
    s = _spectral([1] * 6)
    send, rec = ["c2", "c0"], ["c0", "c3", "c2"]
    res = spy.connectivityanalysis(s, channelcmb=[send, rec], **on_emulator(method))
    assert res.data.shape == (1, 3, 2, 3) and list(res.channel_i) == send and list(res.channel_j) == rec
    S = PO.cross_spectra(np.asarray(s.data))[0].astype(np.complex64)
    want = PO.measures(S)[method][:, [2, 0], :][:, :, [0, 3, 2]]
    sub = S[:, :, [2, 0], :][:, :, :, [0, 3, 2]]
    if method == "plv":
        assert np.allclose(res.data[0], want, rtol=1e-4, atol=2e-5)
    else:
        # the zero diagonal stays where sender equals receiver: (c2, c2) and (c0, c0)
        assert res.data[0, :, 0, 2].tolist() == [0, 0, 0] and res.data[0, :, 1, 0].tolist() == [0, 0, 0]
        tol = PO.bounds(sub)[method]
        assert np.all(np.abs(res.data[0] - want) <= tol)
        if method != "pli":                                                               # (|N| may well be 0 elsewhere)
            assert np.count_nonzero(res.data[0]) == 3 * 4
    by_index = spy.connectivityanalysis(s, channelcmb=[[2, 0], [0, 3, 2]], **on_emulator(method))
    assert np.array_equal(by_index.data, res.data)
