"""The envelope correlations (amplcorr, powcorr, powcorr_ortho: syncopy_amd/csrc/envcorr.hip, envcorr_kernel.h) without a
GPU: the model's own conventions, the library's launchers and kernels through the CPU emulation
(tests/emu/envcorr_emu.cpp) at the kernel shapes of tests/envcorr_oracle.py under its bounds, every refusal of the
launchers, and the rules of the front end that are decided before the device is needed (the measures have no per-trial
engine route; the front end itself is tested on the device, tests/test_gpu_envcorr.py)."""
import functools

import numpy as np
import pytest

import build_emu
import csd_drive as D
import envcorr_oracle as EO
import syncopy_amd as spy
from oracle_routines import ORACLE_CONN
from syncopy_amd.shared.errors import SPYValueError

ptr = D.ptr


@functools.lru_cache(None)
def lib():
    return build_emu.emulated_library("envcorr")


@functools.lru_cache(None)
def ctx(lds_per_block=0):
    c = build_emu.ctx(lib())
    lib().emu_ctx_set_chip(c, D.NO_RECUT, lds_per_block)
    return c


def accumulators(measure, F, Cn):
    return np.zeros((EO.PLANES[measure], F, Cn, Cn)), np.zeros((F, Cn, 2))


def accumulate(spec, measure, pair, chan, split=None):
    """spyhip_envcorr_accumulate on spec (T, K, F, C) complex64, in launches of `split` trials"""
    T, K, F, Cn = spec.shape
    t0 = 0
    for n in split or [T]:
        part = np.ascontiguousarray(spec[t0:t0 + n])
        assert lib().spyhip_envcorr_accumulate(ctx(), ptr(part), n, K, F, Cn, EO.MEASURE_CODE[measure], ptr(pair), ptr(chan)) == 0
        t0 += n
    assert t0 == T


def finalize(pair, chan, nrep, measure):
    _, F, Cn, _ = pair.shape
    out = np.full((F, Cn, Cn), np.nan, dtype=np.float32)
    assert lib().spyhip_envcorr_finalize(ctx(), ptr(pair), ptr(chan), F, Cn, nrep, EO.MEASURE_CODE[measure], ptr(out)) == 0
    return out


@functools.lru_cache(None)
def case(shape):
    """spectra and the three models of a kernel shape, computed once and left unchanged"""
    spec = EO.spectra(*shape)
    spec.setflags(write=False)
    return spec, {m: EO.model(spec, m) for m in EO.MEASURES}


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_model_hand_check():
    """two channels, R = 3: x_0 = (1, 2, 3), x_1 = (2j, 2j, 4j)"""
    spec = np.array([[1, 2j], [2, 2j], [3, 4j]], dtype=np.complex64).reshape(3, 1, 1, 2)
    m = EO.measures(spec)
    # amplitudes (1, 2, 3) and (2, 2, 4): cov = 18 - 6 * 8 / 3 = 2, va = 14 - 12 = 2, vb = 24 - 64 / 3 = 8 / 3
    assert m["amplcorr"][0, 0, 1] == pytest.approx(2 / np.sqrt(2 * 8 / 3)) and np.all(m["amplcorr"][0, [0, 1], [0, 1]] == 1)
    # powers (1, 4, 9) and (4, 4, 16): cov = 164 - 14 * 24 / 3 = 52, va = 98 - 196 / 3, vb = 288 - 192 = 96
    assert m["powcorr"][0, 0, 1] == pytest.approx(52 / np.sqrt((98 - 196 / 3) * 96))
    # orthogonal phases: s = Im(x_0 conj(x_1)) = -|x_0| |x_1|, q_1|0 = p_1 and q_0|1 = p_0: both directions are powcorr
    assert m["powcorr_ortho"][0, 0, 1] == pytest.approx(m["powcorr"][0, 0, 1]) and not m["powcorr_ortho"][0, [0, 1], [0, 1]].any()
    # equal phases: nothing of either channel is orthogonal to the other
    spec = np.array([[1 + 1j, 2 + 2j], [2 + 2j, 2 + 2j], [3 + 3j, 4 + 4j]], dtype=np.complex64).reshape(3, 1, 1, 2)
    assert not EO.measures(spec)["powcorr_ortho"].any()
    assert EO.gamma(3) == pytest.approx(3 * 2.0 ** -24, rel=1e-6)


def test_model_conventions():
    spec = EO.spectra(6, 3, 5, 2)
    x = spec.reshape(10, 3, 6).astype(np.complex128)
    for name in EO.MEASURES:
        mod = EO.model(spec, name)
        r = mod["want"]
        assert np.array_equal(r, r.transpose(0, 2, 1)) and np.all(np.abs(r) <= 1), name
        assert not r[:, 4:, :].any() and not r[:, :, 4:].any(), name                 # the constant and the dead channel
        assert np.all(r[:, :4, :4][:, ~np.eye(4, dtype=bool)] != 0), name
        assert np.all(np.isfinite(mod["tol"][:, :4, :4][:, ~np.eye(4, dtype=bool)])), name
        # a positive scale per channel changes nothing
        scaled = (x * np.array([1, 2, 0.5, 4, 1, 1])).reshape(5, 2, 3, 6).astype(np.complex64)
        assert np.allclose(EO.model(scaled, name)["want"], r, rtol=0, atol=1e-6), name
    i = np.arange(6)
    for name in ("amplcorr", "powcorr"):
        r = EO.model(spec, name)["want"]
        assert np.all(r[:, i[:4], i[:4]] == 1) and not r[:, i[4:], i[4:]].any(), name
        e = np.abs(x[..., :4]) ** (1 if name == "amplcorr" else 2)
        for f in range(3):
            assert np.allclose(r[f, :4, :4], np.corrcoef(e[:, f].T), rtol=0, atol=1e-12), name
    # Hipp's form: the power of j orthogonal to i is |Im(x_j conj(x_i) / |x_i|)|^2
    r = EO.model(spec, "powcorr_ortho")["want"]
    p = np.abs(x) ** 2
    for a, b in ((0, 1), (2, 3), (3, 0)):
        qba = np.imag(x[..., b] * np.conj(x[..., a]) / np.abs(x[..., a])) ** 2
        qab = np.imag(x[..., a] * np.conj(x[..., b]) / np.abs(x[..., b])) ** 2
        for f in range(3):
            want = 0.5 * (np.corrcoef(p[:, f, a], qba[:, f])[0, 1] + np.corrcoef(p[:, f, b], qab[:, f])[0, 1])
            assert r[f, a, b] == pytest.approx(want, abs=1e-12)
    assert not r[:, i, i].any()


# ---- launchers and kernels on the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["one launch", "two launches"])
@pytest.mark.parametrize("shape", EO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernels_at_dispatch_edges(shape, split):
    Cn, F, T, K = shape
    spec, models = case(shape)
    nt = (Cn + 31) // 32
    got = {}
    for m in EO.MEASURES:
        pair, chan = accumulators(m, F, Cn)
        build_emu.launches(lib())
        accumulate(spec, m, pair, chan, [1, T - 1] if split else None)
        log = build_emu.launches(lib())
        staged = 16 if m == "powcorr_ortho" else 8
        assert log[:, [0, 3, 6]].tolist() == [[8 * ((F + 7) // 8) * nt * (nt + 1) // 2, 256, 2 * 2 * K * 32 * staged]] * (2 if split else 1)
        got[m] = finalize(pair, chan, T * K, m)
        # only the lower triangle at tile granularity is maintained
        for bi in range(nt):
            for bj in range(bi + 1, nt):
                assert not pair[:, :, 32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32].any()
        # the per-channel sums are formed once per launch: they are the diagonal of the pair sums for amplcorr / powcorr
        if m != "powcorr_ortho":
            assert np.array_equal(chan[:, :, 1], pair[0][:, np.arange(Cn), np.arange(Cn)])
        assert not chan[:, Cn - 1].any() and np.all(chan[:, :Cn - 1, 0] > 0)
    EO.check(got, spec, what="emulator " + "-".join(map(str, shape)) + (" split" if split else ""), models=models)
    for m in EO.MEASURES:                      # the dead and the constant channel: exact zeros, their diagonal included
        assert not got[m][:, Cn - 2:, :].any() and not got[m][:, :, Cn - 2:].any(), m


def test_finalize_reads_the_lower_triangle_only():
    spec, models = case((33, 3, 4, 1))
    for m in EO.MEASURES:
        pair, chan = accumulators(m, 3, 33)
        accumulate(spec, m, pair, chan)
        want = finalize(pair, chan, 4, m)
        pair[:, :, np.triu(np.ones((33, 33), dtype=bool), 1)] = np.nan
        if m == "powcorr_ortho":
            pair[:, :, np.arange(33), np.arange(33)] = 1e-9                    # a rounding residue on the diagonal
        assert np.array_equal(finalize(pair, chan, 4, m), want), m
    # the clamp: sums that would give 1 + 2e-16 or worse
    pair, chan = np.full((1, 1, 2, 2), 14.0 + 1e-14), np.array([[[6.0, 14.0], [6.0, 14.0]]])
    assert finalize(pair, chan, 3, "amplcorr").tolist() == [[[1.0, 1.0], [1.0, 1.0]]]
    pair[:] = 10.0 - 1e-14
    assert finalize(pair, chan, 3, "powcorr")[0, 1, 0] == -1.0
    # the zero-variance rule: E2 - E1^2 / R = 2^-41 E2 counts as zero, 2^-39 E2 does not
    for k, want in ((-41, 0.0), (-39, 1.0)):
        chan = np.array([[[3.0, 3.0 / (1 - 2.0 ** k)], [6.0, 14.0]]])
        assert finalize(np.ones((1, 1, 2, 2)), chan, 3, "powcorr")[0, 0, 0] == want


def test_launchers_refuse():
    L, c = lib(), ctx()
    spec = EO.spectra(5, 3, 2, 2)
    pair, chan = accumulators("powcorr_ortho", 3, 5)
    accumulate(spec, "powcorr_ortho", pair, chan)
    keep = pair.copy(), chan.copy()
    out = np.full((3, 5, 5), 9.0, dtype=np.float32)
    s, p, ch, o = ptr(spec), ptr(pair), ptr(chan), ptr(out)
    build_emu.launches(L)
    acc, fin = L.spyhip_envcorr_accumulate, L.spyhip_envcorr_finalize
    # null arguments
    assert [acc(None, s, 2, 2, 3, 5, 2, p, ch), acc(c, None, 2, 2, 3, 5, 2, p, ch), acc(c, s, 2, 2, 3, 5, 2, None, ch),
            acc(c, s, 2, 2, 3, 5, 2, p, None), fin(None, p, ch, 3, 5, 4, 2, o), fin(c, None, ch, 3, 5, 4, 2, o),
            fin(c, p, None, 3, 5, 4, 2, o), fin(c, p, ch, 3, 5, 4, 2, None)] == [-1] * 8
    # shapes
    assert [acc(c, s, -1, 2, 3, 5, 2, p, ch), acc(c, s, 2, 0, 3, 5, 2, p, ch), acc(c, s, 2, 2, 0, 5, 2, p, ch),
            acc(c, s, 2, 2, 3, 0, 2, p, ch), fin(c, p, ch, 0, 5, 4, 2, o), fin(c, p, ch, 3, 0, 4, 2, o)] == [-1] * 6
    # a measure that is none; fewer than two repetitions
    assert [acc(c, s, 2, 2, 3, 5, 3, p, ch), acc(c, s, 2, 2, 3, 5, -1, p, ch), fin(c, p, ch, 3, 5, 4, 3, o),
            fin(c, p, ch, 3, 5, 4, -1, o), fin(c, p, ch, 3, 5, 1, 2, o), fin(c, p, ch, 3, 5, 0, 2, o)] == [-1] * 6
    # tapers that do not fit the LDS staging buffer.  1 KiB holds the two buffers of one taper for amplcorr and powcorr
    # and of none for powcorr_ortho, whose staged element is twice as wide
    small = ctx(lds_per_block=1024)
    assert [acc(small, s, 2, 2, 3, 5, m, p, ch) for m in (0, 1, 2)] == [-3] * 3
    assert acc(small, s, 4, 1, 3, 5, 2, p, ch) == -3
    assert len(build_emu.launches(L)) == 0                                      # nothing ran
    assert np.array_equal(pair, keep[0]) and np.array_equal(chan, keep[1]) and np.all(out == 9.0)
    one = accumulators("powcorr", 3, 5)
    assert acc(small, s, 4, 1, 3, 5, 1, ptr(one[0]), ptr(one[1])) == 0 and one[0].any() and one[1].any()
    assert acc(ctx(lds_per_block=2048), s, 4, 1, 3, 5, 2, p, ch) == 0 and not np.array_equal(pair, keep[0])
    build_emu.launches(L)
    # no trials: nothing to do
    keep = pair.copy(), chan.copy()
    assert acc(c, s, 0, 2, 3, 5, 2, p, ch) == 0 and len(build_emu.launches(L)) == 0
    assert np.array_equal(pair, keep[0]) and np.array_equal(chan, keep[1])
    assert fin(c, p, ch, 3, 5, 2, 2, o) == 0 and np.all(np.abs(out) <= 1)


# ---- the front end ----------------------------------------------------------------------------------------------------------------
def _analog(nchan=4, ntrials=5, nsamples=120, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(ntrials * nsamples, nchan)).astype(np.float32)
    return spy.AnalogData(x, samplerate=100.0, trialdefinition=[[k * nsamples, (k + 1) * nsamples, 0] for k in range(ntrials)])


def test_method_names():
    from syncopy_amd.shared.const_def import connectivityMethods, envelopeMethods
    assert envelopeMethods == EO.MEASURES and set(EO.MEASURES) <= set(connectivityMethods)
    from syncopy_amd import _lib, abi, backend
    for fn in ("spyhip_envcorr_accumulate", "spyhip_envcorr_finalize"):
        assert fn in _lib.SIGNATURES and hasattr(lib(), fn)
    assert abi.ENVCORR_MEASURE == backend.ENVCORR_MEASURE == EO.MEASURE_CODE and backend.ENVCORR_PLANES == EO.PLANES
    with pytest.raises(SPYValueError, match="powcorr_ortho"):
        spy.connectivityanalysis(_analog(), method="powcorr_orth")


@pytest.mark.parametrize("method", EO.MEASURES)
def test_rules_decided_before_the_device(method):
    d = _analog()
    for keep in (True, "yes", 1):
        with pytest.raises(SPYValueError, match="trial averaging needed for method " + method):
            spy.connectivityanalysis(d, method=method, keeptrials=keep)
    one = spy.AnalogData(np.zeros((100, 2), "f4"), samplerate=100)
    with pytest.raises(SPYValueError, match="only one trial"):
        spy.connectivityanalysis(one, method=method)
    with pytest.raises(SPYValueError, match="only one trial"):
        spy.connectivityanalysis(d, method=method, select={"trials": [2]})
    with pytest.raises(SPYValueError, match="noise weighting exists for the methods"):
        spy.connectivityanalysis(d, method=method, noise_weighted=True)
    # no per-trial engine route: single-trial cross spectra are summed over the tapers
    for how in ("sequential", "parallel"):
        with pytest.raises(NotImplementedError, match="batched route only"):
            spy.connectivityanalysis(d, method=method, compute_method=how, routine_classes=ORACLE_CONN)
    with pytest.warns(UserWarning, match="Jackknife is not available for method " + method):
        with pytest.raises(NotImplementedError):
            spy.connectivityanalysis(d, method=method, jackknife=True, compute_method="sequential", routine_classes=ORACLE_CONN)
