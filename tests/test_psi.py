"""The phase slope index (syncopy_amd/csrc/phaseslope.hip, phaseslope_kernel.h) without a GPU: the model's own conventions,
the library's launchers and kernels through the CPU emulation (tests/emu/phaseslope_emu.cpp) at the kernel shapes of
tests/psi_oracle.py under its bound, every refusal of the launchers, and the rules of the front end that are decided before
the device is needed (the front end itself is tested on the device, tests/test_gpu_psi.py)."""
import functools

import numpy as np
import pytest

import build_emu
import csd_drive as D
import psi_oracle as PO
import syncopy_amd as spy
from syncopy_amd.shared.errors import SPYValueError

ptr = D.ptr
FOURIER = 2     # SPYHIP_OUT_FOURIER


@functools.lru_cache(None)
def lib():
    return build_emu.emulated_library("phaseslope")


@functools.lru_cache(None)
def ctx():
    return build_emu.ctx(lib())


def phaseslope(csd, half, raw=False, fill=np.nan, planes=None):
    """spyhip_phaseslope on the Hermitian csd (F, C, C), or spyhip_phaseslope_from_accumulator on its raw accumulator"""
    F, Cn = csd.shape[:2]
    out = np.full((planes or (F if half else 1), Cn, Cn), fill, dtype=np.float32)
    if raw:
        acc = PO.raw_accumulator(csd)
        keep = acc.copy()
        assert lib().spyhip_phaseslope_from_accumulator(ctx(), ptr(acc), F, Cn, PO.SCALE, half, ptr(out)) == 0
        assert np.array_equal(acc.view(np.uint32), keep.view(np.uint32))            # not modified
    else:
        assert lib().spyhip_phaseslope(ctx(), ptr(csd), F, Cn, half, ptr(out)) == 0
    return out


def coh_normalize(csd):
    """spyhip_coh_normalize (output 'fourier') of the emulated cross-spectral library"""
    F, Cn = csd.shape[:2]
    out = np.zeros((F, Cn, Cn), dtype=np.complex64)
    with np.errstate(all="ignore"):
        assert D.lib().spyhip_coh_normalize(D.ctx(), ptr(csd), F, Cn, FOURIER, ptr(out)) == 0
    return out


@functools.lru_cache(None)
def case(Cn, F):
    """the CSD of a kernel shape and K5's coherency of it, computed once and left unchanged"""
    csd = PO.hermitian_csd(PO.spectra(Cn, F))
    coh = coh_normalize(csd)
    csd.setflags(write=False)
    coh.setflags(write=False)
    return csd, coh


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_model_hand_check():
    """one pair whose phase advances by 0.1 rad per bin at coherence 0.5: every edge is 0.25 sin 0.1"""
    F = 7
    c = np.zeros((F, 2, 2), dtype=np.complex64)
    c[:, 0, 0] = c[:, 1, 1] = 1
    c[:, 0, 1] = 0.5 * np.exp(0.1j * np.arange(F))
    c[:, 1, 0] = np.conj(c[:, 0, 1])
    m = PO.psi_model(c, 2)
    assert np.isnan(m[[0, 1, 5, 6]]).all() and np.allclose(m[2:5, 0, 1], 4 * 0.25 * np.sin(0.1), rtol=1e-6)
    assert np.array_equal(m[2:5], -m[2:5].transpose(0, 2, 1)) and not m[2:5, [0, 1], [0, 1]].any()
    whole = PO.psi_model(c, 0)
    assert whole.shape == (1, 2, 2) and whole[0, 0, 1] == pytest.approx(6 * 0.25 * np.sin(0.1), rel=1e-6)
    c[3, 0, 1] = np.nan                                       # non-finite coherency counts as 0: two edges drop out
    assert PO.psi_model(c, 0)[0, 0, 1] == pytest.approx(4 * 0.25 * np.sin(0.1), rel=1e-6)


def test_model_sign_of_a_delay():
    """S_ij = <x_i conj(x_j)> with x_j = x_i delayed: the phase of S_ij grows with frequency, psi[i, j] > 0 (i leads j)"""
    F = 16
    f = np.arange(F)
    c = np.zeros((F, 2, 2), dtype=np.complex64)
    c[:, 0, 0] = c[:, 1, 1] = 1
    c[:, 0, 1] = 0.8 * np.exp(2j * np.pi * f * 1.0 / 64)     # x_1(f) = x_0(f) exp(-2 pi i f d / N)
    c[:, 1, 0] = np.conj(c[:, 0, 1])
    m = PO.psi_model(c, 3)
    assert np.all(m[3:13, 0, 1] > 0) and np.all(m[3:13, 1, 0] < 0)


# ---- the kernels, emulated ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PO.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernel_shapes(shape):
    Cn, F, half = shape
    csd, coh = case(Cn, F)
    build_emu.launches(lib())
    got = phaseslope(csd, half)
    rows = build_emu.launches(lib())
    nt = (Cn + 31) // 32
    assert rows[0, 0] == nt * (nt + 1) // 2 * PO.RUNS.get(shape, 1) and rows[0, 3] == 256, rows     # the frequency runs
    assert len(rows) == (2 if half == 0 and PO.RUNS.get(shape, 1) > 1 else 1)
    PO.check(got, coh, half, what="emulated " + "-".join(map(str, shape)))
    valid = slice(half, F - half) if half else slice(0, 1)
    assert not got[valid, -1, :].any() and not got[valid, :, -1].any()               # the zero channel: exact zeros
    if Cn == 1:
        assert not got[valid].any()
    else:
        assert np.abs(got[valid, :Cn - 1, :Cn - 1]).max() > 0.05                     # not noise
    # the two entries agree bit for bit; the strictly upper tiles of the accumulator are NaN and are not read
    again = phaseslope(csd, half, raw=True)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_half_zero_leaves_the_rest_of_out_alone():
    csd, coh = case(33, 41)
    got = phaseslope(csd, 0, fill=7.5, planes=3)
    assert np.all(got[1:] == 7.5)
    PO.check(got[:1], coh, 0, what="emulated 33-41-0, three planes given")


def test_refusals():
    csd, _ = case(33, 9)
    out = np.full((9, 33, 33), 3.5, dtype=np.float32)
    L, c = lib(), ctx()
    for fn, scale in ((L.spyhip_phaseslope, ()), (L.spyhip_phaseslope_from_accumulator, (1.0,))):
        assert fn(c, ptr(csd), 9, 33, *scale, 4, ptr(out)) == 0                      # 2h = F - 1 fits: one valid bin
        out[:] = 3.5
        for args in ((None, ptr(csd), 9, 33, *scale, 1, ptr(out)), (c, None, 9, 33, *scale, 1, ptr(out)),
                     (c, ptr(csd), 9, 33, *scale, 1, None), (c, ptr(csd), 0, 33, *scale, 1, ptr(out)),
                     (c, ptr(csd), 1, 33, *scale, 0, ptr(out)), (c, ptr(csd), 9, 0, *scale, 1, ptr(out)),
                     (c, ptr(csd), 9, -3, *scale, 1, ptr(out)), (c, ptr(csd), 9, 33, *scale, -1, ptr(out)),
                     (c, ptr(csd), 9, 33, *scale, 5, ptr(out)), (c, ptr(csd), 2, 33, *scale, 1, ptr(out))):
            assert fn(*args) == -1, args
        assert np.all(out == 3.5)


def test_entries_are_declared():
    from syncopy_amd import _lib
    header = open(build_emu.ROOT + "/include/spyhip.h").read()
    for fn in ("spyhip_phaseslope", "spyhip_phaseslope_from_accumulator"):
        assert fn in _lib.SIGNATURES and "int " + fn + "(" in header and hasattr(lib(), fn)


# ---- the front end, before the device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    trl = np.stack([np.arange(4) * 100, np.arange(1, 5) * 100, np.zeros(4)], axis=1)
    return spy.AnalogData(rng.normal(size=(400, 3)).astype(np.float32), samplerate=100.0, trialdefinition=trl)


def test_method_sets():
    from syncopy_amd.shared import const_def as cd
    assert "psi" in cd.connectivityMethods
    assert "psi" not in cd.phaseMethods + cd.directedMethods + cd.envelopeMethods


def test_front_end_rules(data):
    with pytest.raises(SPYValueError, match="bandwidth"):
        spy.connectivityanalysis(data, method="coh", bandwidth=8)
    for bad in (0, -2.0, "wide", True, float("nan")):
        with pytest.raises(SPYValueError, match="bandwidth"):
            spy.connectivityanalysis(data, method="psi", bandwidth=bad)
    with pytest.raises(SPYValueError, match="trial averaging needed for method psi"):
        spy.connectivityanalysis(data, method="psi", keeptrials=True)
    with pytest.raises(SPYValueError, match="only one trial"):
        spy.connectivityanalysis(data, method="psi", select={"trials": [1]})
    with pytest.raises(SPYValueError, match="equidistant"):
        spy.connectivityanalysis(data, method="psi", foi=[5, 6, 7, 9, 12], bandwidth=2)
    with pytest.raises(SPYValueError, match="does not fit"):
        spy.connectivityanalysis(data, method="psi", foilim=[10, 20], bandwidth=11)      # h = 6 > (11 - 1) / 2
    with pytest.raises(SPYValueError, match="noise weighting exists for the methods"):
        spy.connectivityanalysis(data, method="psi", noise_weighted=True)
