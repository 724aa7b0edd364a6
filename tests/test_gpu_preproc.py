"""spy.preprocessing on the device (csrc/preproc.hip) against the NumPy / SciPy model (preproc_oracle.py) run through the
same front end, and the ABI wrappers on their own.  Criterion: tests/parity.py per trial.  Detrend order 0 and the z-score
are compared with the float32 NumPy / SciPy result, the filters and the line fit with the float64 model.

Measured on an MI355X: see DESIGN.md section 8 (whether detrend / z-score are bit-identical is printed by
test_demean_and_zscore_bits)."""
import numpy as np
import pytest

import syncopy_amd as spy
import preproc_oracle as PO
from parity import assert_parity, excess

pytestmark = pytest.mark.gpu
HOW = dict(compute_method="sequential", routine_classes=PO.PREPROC_OPS)
FS = 1000.0


def _data(lengths, nchan, seed=0, offset=True):
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    x = rng.normal(size=(total, nchan))
    if offset:
        x += rng.normal(size=(1, nchan)) + np.linspace(0, 1.5, total)[:, None] * rng.normal(size=(1, nchan))
    edges = np.concatenate([[0], np.cumsum(lengths)])
    trl = np.stack([edges[:-1], edges[1:], np.zeros(len(lengths))], axis=1)
    return spy.AnalogData(x.astype(np.float32), samplerate=FS, trialdefinition=trl)


def _compare(data, what, exact=False, **kw):
    got = spy.preprocessing(data, **kw)
    ref = spy.preprocessing(data, **kw, **HOW)
    assert got.data.dtype == np.float32 and got.data.shape == ref.data.shape, what
    assert np.array_equal(np.asarray(got.trialdefinition), np.asarray(ref.trialdefinition)), what
    assert list(got.channel) == list(ref.channel), what
    assert got.info.get("nan_trials") == ref.info.get("nan_trials"), what
    worst = 0.0
    for g, r in zip(got.trials, ref.trials):
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(g), nan), f"{what}: NaN pattern"
        if (~nan).any():
            worst = max(worst, excess(g[~nan], r[~nan]))
    print(f"{what}: err/tol {worst:.3g}")
    assert worst <= 1.0, f"{what}: err/tol {worst:.3g}"
    if exact:
        print(f"{what}: bit-identical {np.array_equal(got.data, ref.data, equal_nan=True)}")
    return got, ref


@pytest.mark.parametrize("ftype,freq", [("lp", 100), ("hp", 30), ("bp", [20, 80]), ("bs", [45, 55])])
@pytest.mark.parametrize("direction", ["twopass", "onepass"])
@pytest.mark.parametrize("order", [4, 6])
def test_butterworth(ftype, freq, direction, order):
    data = _data([700, 512, 700, 333], 70, seed=order)
    _compare(data, f"but {ftype} {direction} {order}", filter_class="but", filter_type=ftype, freq=freq, order=order,
             direction=direction)


@pytest.mark.parametrize("ftype,freq", [("lp", 100), ("hp", 30), ("bp", [20, 80]), ("bs", [45, 55])])
@pytest.mark.parametrize("direction", ["twopass", "onepass", "onepass-minphase"])
def test_firws_types_and_directions(ftype, freq, direction):
    data = _data([300, 257, 300], 70, seed=3)
    _compare(data, f"firws {ftype} {direction}", filter_class="firws", filter_type=ftype, freq=freq, order=60,
             direction=direction)


@pytest.mark.parametrize("window", ["hamming", "hann", "blackman"])
@pytest.mark.parametrize("order", [50, 51])
def test_firws_windows_even_and_odd_order(window, order):
    data = _data([400], 5, seed=4)
    _compare(data, f"firws {window} {order}", filter_class="firws", filter_type="lp", freq=120, order=order, window=window,
             direction="onepass")


# the FIR tile is 128 outputs x 64 channels, 128 taps per stage: lengths and tap counts at and next to those
@pytest.mark.parametrize("nsamp", [127, 128, 129, 255, 256, 257])
@pytest.mark.parametrize("nchan", [1, 63, 64, 65])
def test_firws_tile_boundaries(nsamp, nchan):
    data = _data([nsamp, nsamp], nchan, seed=nsamp + nchan)
    for order in (126, 128, 256):
        _compare(data, f"firws n={nsamp} c={nchan} order={order}", filter_class="firws", filter_type="lp", freq=100,
                 order=order, direction="onepass")


def test_firws_order_1000_on_4096_and_default_order_on_short_trial():
    data = _data([4096, 4096], 70, seed=6)
    _compare(data, "firws order 1000", filter_class="firws", filter_type="bp", freq=[8, 30], order=1000, direction="onepass")
    short = _data([200, 200], 6, seed=7)
    got, _ = _compare(short, "firws order = trial length", filter_class="firws", filter_type="lp", freq=60, direction="onepass")
    assert got.cfg["preprocessing"]["order"] is None


def test_firws_notch_with_line_noise():
    """white noise of unit variance plus a 50 Hz line of amplitude 100 at 1 kHz, bs 45-55 Hz, order 1000, Hamming"""
    rng = np.random.default_rng(50)
    t = np.arange(4096) / FS
    x = rng.normal(size=(4096, 8)) + 100.0 * np.sin(2 * np.pi * 50.0 * t[:, None] + rng.uniform(0, 6, size=(1, 8)))
    data = spy.AnalogData(x.astype(np.float32), samplerate=FS)
    _compare(data, "firws notch", filter_class="firws", filter_type="bs", freq=[45, 55], order=1000, window="hamming",
             direction="onepass")


@pytest.mark.parametrize("kw", [dict(filter_class=None, polyremoval=0), dict(filter_class=None, zscore=True),
                                dict(filter_class=None, polyremoval=0, zscore=True)])
@pytest.mark.parametrize("nchan", [1, 5, 70])
def test_demean_and_zscore_bits(kw, nchan):
    data = _data([4096, 1000, 130, 7], nchan, seed=8)
    data.data[:4096] += (3.0 + np.linspace(0, 8, 4096))[:, None].astype(np.float32)
    data.invalidate()
    _compare(data, f"{kw} c={nchan}", exact=True, **kw)


@pytest.mark.parametrize("kw", [dict(filter_class=None, polyremoval=1), dict(filter_class=None, polyremoval=1, zscore=True),
                                dict(polyremoval=0, freq=80), dict(polyremoval=1, freq=80, zscore=True),
                                dict(filter_class="firws", polyremoval=1, freq=80, order=100, zscore=True),
                                dict(filter_class="firws", polyremoval=0, freq=80, order=100, rectify=True),
                                dict(freq=80, rectify=True), dict(filter_class=None, zscore=True, rectify=True),
                                dict(filter_class=None, polyremoval=1, rectify=True),
                                dict(freq=[20, 60], filter_type="bp", direction="onepass", rectify=True)])
def test_chains(kw):
    _compare(_data([600, 450, 600], 33, seed=9), f"chain {kw}", **kw)


def test_unequal_lengths_selection_and_chunks(monkeypatch):
    import importlib
    mod = importlib.import_module("syncopy_amd.preproc.preprocessing")
    data = _data([500, 300, 500, 301, 300, 500], 70, seed=10)
    sel = {"trials": [4, 0, 2, 1], "channel": [3, 1, 60], "latency": [0.05, 0.28]}
    for kw in (dict(freq=90), dict(filter_class="firws", freq=90, order=80), dict(filter_class=None, zscore=True)):
        full = spy.preprocessing(data, **kw)
        _compare(data, f"unequal {kw}", **kw)
        _compare(data, f"select {kw}", select=sel, **kw)
        monkeypatch.setattr(mod, "CHUNK_BYTES", 500 * 70 * 4)          # one trial per launch
        small = spy.preprocessing(data, **kw)
        monkeypatch.undo()
        assert np.array_equal(full.data, small.data), kw


@pytest.mark.parametrize("kw", [dict(filter_class="firws", freq=90, order=40, direction="onepass"),
                                dict(filter_class="firws", freq=90, order=40, direction="twopass"),
                                dict(freq=90), dict(filter_class=None, polyremoval=1), dict(filter_class=None, polyremoval=0)])
def test_nan_in_one_channel_of_one_trial(kw):
    data = _data([400, 400, 400], 9, seed=11)
    data.data[400 + 123, 4] = np.nan
    data.invalidate()
    with pytest.warns(UserWarning, match="NaN"):
        got = spy.preprocessing(data, **kw)
    assert got.info["nan_trials"] == [1]
    with pytest.warns(UserWarning, match="NaN"):
        _, ref = _compare(data, f"nan {kw}", **kw)
    bad = np.isnan(ref.data)
    assert bad[:, [c for c in range(9) if c != 4]].sum() == 0 and bad[:400].sum() == 0 and bad[800:].sum() == 0
    if kw.get("filter_class") == "firws":
        reach = 41 if kw["direction"] == "onepass" else 81
        assert bad.sum() == reach


def test_device_resident_input_and_freqanalysis_chain():
    from oracle_routines import ORACLE_FREQ
    data = _data([1000] * 5, 16, seed=12)
    host = spy.preprocessing(data, filter_type="bp", freq=[10, 200])
    data.device_data()
    keep = data._data
    data._data = None                                   # the host array is out of reach: only the device copy can serve
    data.set_pending(lambda: (_ for _ in ()).throw(AssertionError("host copy read")), keep.shape, keep.dtype)
    dev = spy.preprocessing(data, filter_type="bp", freq=[10, 200])
    assert np.array_equal(dev.data, host.data)
    filt = spy.preprocessing(_data([1000] * 5, 16, seed=12), filter_type="bp", freq=[10, 200])
    assert filt._device is not None and filt._data is None
    spec = spy.freqanalysis(filt, method="mtmfft", tapsmofrq=3)
    ref_f = spy.preprocessing(_data([1000] * 5, 16, seed=12), filter_type="bp", freq=[10, 200], **HOW)
    ref = spy.freqanalysis(ref_f, method="mtmfft", tapsmofrq=3, compute_method="sequential", routine_classes=ORACLE_FREQ)
    assert_parity(spec.data, ref.data, what="preprocessing -> mtmfft")


def test_abi_wrappers_directly():
    import torch
    from syncopy_amd import backend
    from syncopy_amd.preproc import design
    rng = np.random.default_rng(13)
    x = rng.normal(size=(3, 300, 10)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    nan = torch.zeros(3, dtype=torch.int32, device="cuda")
    sos, zi, edge = design.butterworth(4, [20, 80], "bp", FS)
    out = backend.sosfiltfilt(xd, torch.empty_like(xd), sos, zi, edge, nan).cpu().numpy()
    for t in range(3):
        assert_parity(out[t], PO.sosfiltfilt(x[t], sos), what="sosfiltfilt")
    taps = torch.from_numpy(design.windowed_sinc("hann", 500, 0.1)).cuda()          # 501 taps on 300 samples
    out = backend.fir_same(xd, torch.empty_like(xd), taps, nan, rectify=True).cpu().numpy()
    for t in range(3):
        assert_parity(out[t], np.abs(PO.fir64(x[t], taps.cpu().numpy())), what="fir_same")
    out = backend.detrend(xd.clone(), torch.empty_like(xd), 0, nan).cpu().numpy()
    assert_parity(out[0], PO.detrend(x[0], 0), what="detrend")
    assert not nan.any().item()
    with pytest.raises(backend.SpyHipError):
        backend.sosfiltfilt(xd, torch.empty_like(xd), sos, zi, 300, nan)


def test_issue_examples():
    data = _data([3000, 3000], 12, seed=14)
    a = spy.preprocessing(data, filter_class="firws", filter_type="bs", freq=[49, 51], order=2000)
    b = spy.preprocessing(data, freq=100)
    assert a.data.shape == b.data.shape == data.data.shape and np.isfinite(a.data).all() and np.isfinite(b.data).all()
