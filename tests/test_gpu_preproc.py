"""spy.preprocessing on the device (csrc/preproc.hip) against the NumPy / SciPy model (preproc_oracle.py) run through the
same front end, and the ABI wrappers on their own.  Criterion: tests/parity.py per trial.  Detrend order 0 and the z-score
are compared with the float32 NumPy / SciPy result, the filters and the line fit with the float64 model.

The Butterworth cascade is held to a second bound, element-wise 2^-23 |ref| + 1e-10 max_t |ref| per channel
(test_preproc.sos_excess): the parity criterion cannot tell a float64 filter state from a float32 one, this bound can.
Its constant was placed on the CPU between two models (test_preproc.py::test_sos_bound_sits_between_the_models: float64
with fused against separate multiply-adds 2.7e-13, float32 state at least 2.0e-8; neither figure is a device figure).
The device's own distance from that bound is what the tests print as "err/bound".

Measured on an MI355X: see DESIGN.md section 8 (whether detrend / z-score are bit-identical is printed by
test_demean_and_zscore_bits)."""
import numpy as np
import pytest

import syncopy_amd as spy
import preproc_oracle as PO
from parity import ATOL_REL, RTOL, assert_parity, excess
from syncopy_amd.preproc import design
from test_preproc import BUT_CASES, BUT_FREQ, but_sections, sos_excess

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


def _compare(data, what, exact=False, tight=False, model_floor=0.0, **kw):
    """The device against the model through the same front end: the same NaN, +inf and -inf elements, the finite ones at
    parity per trial.  tight: the Butterworth bound of test_preproc.sos_excess as well.  model_floor: what the float64
    model's own rounding leaves where the exact result is zero, added to the tolerance (test_detrend_and_zscore_tiny)."""
    got = spy.preprocessing(data, **kw)
    ref = spy.preprocessing(data, **kw, **HOW)
    assert got.data.dtype == np.float32 and got.data.shape == ref.data.shape, what
    assert np.array_equal(np.asarray(got.trialdefinition), np.asarray(ref.trialdefinition)), what
    assert list(got.channel) == list(ref.channel), what
    assert got.info.get("nan_trials") == ref.info.get("nan_trials"), what
    worst = bound = 0.0
    for g, r in zip(got.trials, ref.trials):
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN pattern"
        assert np.array_equal(g == np.inf, r == np.inf), f"{what}: +inf pattern"
        assert np.array_equal(g == -np.inf, r == -np.inf), f"{what}: -inf pattern"
        ok = np.isfinite(r)
        if ok.any() and model_floor:
            tol = RTOL * np.abs(r[ok]) + ATOL_REL * np.abs(r[ok]).max() + model_floor
            worst = max(worst, float((np.abs(g[ok].astype(np.float64) - r[ok]) / tol).max()))
        elif ok.any():
            worst = max(worst, excess(g[ok], r[ok]))
        if tight:
            bound = max(bound, sos_excess(g, r))
    print(f"{what}: err/tol {worst:.3g}" + (f", err/bound {bound:.3g}" if tight else ""))
    assert worst <= 1.0, f"{what}: err/tol {worst:.3g}"
    assert bound <= 1.0, f"{what}: err/bound {bound:.3g}"
    if exact:
        print(f"{what}: bit-identical {np.array_equal(got.data, ref.data, equal_nan=True)}")
    return got, ref


def _but(data, ftype, order, direction, what, **kw):
    return _compare(data, f"but {ftype} order {order} ({but_sections(ftype, order)} sections) {direction} {what}", tight=True,
                    filter_class="but", filter_type=ftype, freq=BUT_FREQ[ftype], order=order, direction=direction, **kw)


# ---- the Butterworth cascade at every compiled instance -----------------------------------------------------------
# NS = 2, 4, 8 and 12 sections are compiled (SPY_SOS_DISPATCH of csrc/preproc_kernel.h); BUT_CASES runs 1 ... 12
# sections, and each NS once more with RECT = true: 2, 4, 8 and 12 sections
RECTIFIED = [("lp", 4), ("bp", 4), ("hp", 16), ("lp", 24), ("bs", 12)]
EVERY = [(f, o, False) for f, o in BUT_CASES] + [(f, o, True) for f, o in RECTIFIED]


@pytest.mark.parametrize("direction", ["onepass", "twopass"])
@pytest.mark.parametrize("ftype,order,rectify", EVERY,
                         ids=[f"{f}{o}-{but_sections(f, o)}sections" + ("-rect" if r else "") for f, o, r in EVERY])
def test_butterworth_every_section_count(ftype, order, rectify, direction):
    edge = design.butterworth(order, BUT_FREQ[ftype], ftype, FS)[2]
    _but(_data([edge + 9, 333], 5, seed=order), ftype, order, direction, f"rectify={rectify}", rectify=rectify)


# 2, 5 (once with a first-order section, which shortens `edge`) and 12 sections
@pytest.mark.parametrize("ftype,order", [("lp", 3), ("lp", 9), ("bp", 5), ("hp", 24), ("bs", 12)],
                         ids=lambda v: str(v))
def test_butterworth_shortest_legal_trial(ftype, order):
    """nsamp = edge + 1: the odd extension at either end reaches the far end of the trial"""
    import torch
    from syncopy_amd import backend
    sos, zi, edge = design.butterworth(order, BUT_FREQ[ftype], ftype, FS)
    _but(_data([edge + 1, edge + 2, edge + 1], 5, seed=order), ftype, order, "twopass", f"nsamp = edge + 1 = {edge + 1}")
    kw = dict(filter_class="but", filter_type=ftype, freq=BUT_FREQ[ftype], order=order, direction="twopass")
    short = _data([edge + 1, edge], 5, seed=order)
    with pytest.raises(ValueError, match="padlen"):
        spy.preprocessing(short, **kw)
    with pytest.raises(ValueError, match="padlen"):
        spy.preprocessing(short, **kw, **HOW)
    xd = torch.zeros((2, edge, 5), dtype=torch.float32, device="cuda")
    out = torch.full_like(xd, 7.0)
    with pytest.raises(backend.SpyHipError):
        backend.sosfiltfilt(xd, out, sos, zi, edge, torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert (out == 7.0).all().item()


@pytest.mark.parametrize("direction", ["onepass", "twopass"])
def test_butterworth_loop_remainders(direction):
    """5 sections, trials of 40 ... 47 samples: every remainder of nsamp (one-pass) and of nsamp + 2 * edge (forward and
    backward pass) modulo LOAD_AHEAD = 8"""
    _but(_data(list(range(40, 48)), 3, seed=40), "bp", 5, direction, "nsamp 40 ... 47")


def _scaled(lengths, nchan, seed):
    """every channel with an offset and a scale of its own, so that no series can stand in for its neighbour"""
    data = _data(lengths, nchan, seed=seed, offset=False)
    rng = np.random.default_rng(seed + 1)
    scale = np.logspace(-1, 1, nchan)[rng.permutation(nchan)]
    data.data[:] = (data.data * scale + 3.0 * np.arange(1, nchan + 1)).astype(np.float32)
    data.invalidate()
    return data


@pytest.mark.parametrize("ftype,order,direction", [("lp", 4, "twopass"), ("bp", 6, "onepass")])
@pytest.mark.parametrize("nchan", [1, 63, 64, 65])
def test_butterworth_series_map(nchan, ftype, order, direction):
    """3 trials x nchan series against the 64 threads of a workgroup (my_series)"""
    data = _scaled([120, 97, 120], nchan, seed=nchan)
    got, ref = _but(data, ftype, order, direction, f"nchan={nchan}")
    series = np.stack([np.asarray(r)[:97].T for r in ref.trials]).reshape(3 * nchan, 97)     # (trial, channel) order
    for a, b in zip(series[:-1], series[1:]):              # a result stored one series off could not pass
        assert excess(a, b) > 1.0


@pytest.mark.parametrize("direction", ["onepass", "twopass"])
@pytest.mark.parametrize("ftype,order", [("lp", 24), ("bs", 12)])
def test_butterworth_12_sections_nan_in_one_channel(ftype, order, direction):
    edge = design.butterworth(order, BUT_FREQ[ftype], ftype, FS)[2]
    n = edge + 9
    data = _data([n, n, n], 9, seed=17)
    data.data[n + n // 2, 4] = np.nan
    data.invalidate()
    with pytest.warns(UserWarning, match="NaN"):
        got, ref = _but(data, ftype, order, direction, "NaN")          # the model's NaN pattern, all else inside the bounds
    assert got.info["nan_trials"] == [1]
    bad = np.isnan(got.data)
    assert bad[:, [c for c in range(9) if c != 4]].sum() == 0 and bad[:n].sum() == 0 and bad[2 * n:].sum() == 0
    assert np.isfinite(got.data[~bad]).all()
    assert bad.sum() == (n - n // 2 if direction == "onepass" else n)


def test_detrend_and_onepass_in_place():
    """"out may be in" (csrc/preproc_kernel.h): the same bits as out of place"""
    import torch
    from syncopy_amd import backend
    x = torch.from_numpy(np.random.default_rng(21).normal(size=(3, 77, 65)).astype(np.float32) + 2.0).cuda()
    flag = torch.zeros(3, dtype=torch.int32, device="cuda")
    sos12 = design.butterworth(12, BUT_FREQ["bs"], "bs", FS)[0]
    sos3 = design.butterworth(5, BUT_FREQ["lp"], "lp", FS)[0]
    calls = [lambda i, o, r=r, k=k: backend.detrend(i, o, k, flag, r) for k in (0, 1) for r in (False, True)]
    calls += [lambda i, o, r=r, k=k: backend.sosfilt(i, o, k, flag, r) for k in (sos3, sos12) for r in (False, True)]
    for call in calls:
        apart = call(x, torch.empty_like(x)).cpu().numpy()
        buf = x.clone()
        assert call(buf, buf) is buf
        assert np.array_equal(buf.cpu().numpy(), apart)
    one = x[:, :, :1].contiguous()                         # one channel: detrend order 0 takes NumPy's pairwise sum
    apart = backend.detrend(one, torch.empty_like(one), 0, flag).cpu().numpy()
    assert np.array_equal(backend.detrend(one, one, 0, flag).cpu().numpy(), apart)
    assert not flag.any().item()


@pytest.mark.parametrize("kw", [dict(freq=100, order=25), dict(filter_type="hp", freq=30, order=25, direction="onepass"),
                                dict(filter_type="bp", freq=[20, 80], order=13),
                                dict(filter_type="bs", freq=[45, 55], order=13, direction="onepass")])
def test_butterworth_13_sections_are_refused_before_any_device_work(kw, monkeypatch):
    import importlib
    import torch
    from syncopy_amd import backend
    from syncopy_amd.shared.errors import SPYValueError
    mod = importlib.import_module("syncopy_amd.preproc.preprocessing")
    monkeypatch.setattr(mod, "_device_run", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(SPYValueError):
        spy.preprocessing(_data([400, 400], 3, seed=25), **kw)
    monkeypatch.undo()
    sos, zi, edge = design.butterworth(kw["order"], kw["freq"], kw.get("filter_type", "lp"), FS)
    assert sos.shape[0] == 13
    xd = torch.zeros((2, 400, 3), dtype=torch.float32, device="cuda")
    out = torch.full_like(xd, 7.0)
    flag = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(backend.SpyHipError):
        backend.sosfilt(xd, out, sos, flag)
    with pytest.raises(backend.SpyHipError):
        backend.sosfiltfilt(xd, out, sos, zi, edge, flag)
    assert (out == 7.0).all().item()


# ---- detrend and z-score at tiny shapes ---------------------------------------------------------------------------
TINY = (1, 2, 7, 8, 9, 16, 17)


def _tiny(nchan):
    """three trials of every length of TINY; the first holds a constant channel (2.5: its mean is exact, the z-score
    0 / 0), the second one of 0.1 (the float32 mean may miss it), the third one of +-1e-30 in turn (its squares underflow,
    standard deviation 0, the z-score +-inf).  One sample per trial gives 0 / 0 everywhere."""
    lengths = [n for n in TINY for _ in range(3)]
    data = _data(lengths, nchan, seed=nchan, offset=False)
    data.data[:] += np.random.default_rng(nchan).normal(size=(1, nchan)).astype(np.float32)
    row = 0
    for n in TINY:
        data.data[row:row + n, 0] = 2.5
        data.data[row + n:row + 2 * n, nchan - 1] = np.float32(0.1)
        data.data[row + 2 * n:row + 3 * n, 0] = np.float32(1e-30) * (1 - 2 * (np.arange(n) % 2))
        row += 3 * n
    data.invalidate()
    return data


@pytest.mark.parametrize("rectify", [False, True])
@pytest.mark.parametrize("kw", [dict(polyremoval=0), dict(polyremoval=1), dict(zscore=True), dict(polyremoval=0, zscore=True)],
                         ids=lambda kw: "-".join(f"{k}{int(v)}" for k, v in kw.items()))
@pytest.mark.parametrize("nchan", [1, 2, 64, 65])
def test_detrend_and_zscore_tiny(nchan, kw, rectify):
    """nsamp 1, 2, 7, 8, 9, 16, 17 (LOAD_AHEAD = 8, NumPy's pairwise blocks of 8 with one channel) x nchan 1, 2, 64, 65.

    Where the least-squares line meets every sample (one or two samples, a constant channel) the exact result is 0: the
    kernel returns 0, the float64 model what its own rounding leaves (3e-15 at most on these data with the kernel's CPU
    emulation, for samples of size 5: a few 2^-53 of the sample; not a device figure).  The line fit is therefore given
    2^-44 max|x| on top of the parity tolerance: a hundred times that residue, and 1e-6 of the last bit a float32
    result of the samples' size has."""
    data = _tiny(nchan)
    floor = 2.0 ** -44 * float(np.abs(data.data).max()) if kw.get("polyremoval") == 1 else 0.0
    got, ref = _compare(data, f"tiny c={nchan} {kw} rectify={rectify}", model_floor=floor, filter_class=None, rectify=rectify, **kw)
    if kw.get("zscore"):
        odd = ~np.isfinite(ref.data)
        assert np.isnan(ref.data).any() and np.isinf(ref.data).any()
        assert np.array_equal(got.data[odd], ref.data[odd], equal_nan=True)


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
