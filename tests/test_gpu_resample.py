"""spy.resampledata on the device (csrc/resample.hip) against the NumPy / SciPy model (resample_oracle.py) run through the
same front end, against the recorded results of the reference (tests/golden/resample.npz), and the ABI wrapper on its
own.  Criterion: tests/parity.py per trial.

Measured on an MI355X (tools/resample_bench.py): see DESIGN.md section 8."""
import warnings

import numpy as np
import pytest

import syncopy_amd as spy
import resample_oracle as RO
from parity import assert_parity, excess
from test_resample import G, golden_cases

pytestmark = pytest.mark.gpu
HOW = dict(compute_method="sequential", routine_classes=RO.RESAMPLE_OPS)


def _data(lengths, nchan, seed=0, fs=1000.0):
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    x = rng.normal(size=(total, nchan)) + rng.normal(size=(1, nchan))
    edges = np.concatenate([[0], np.cumsum(lengths)])
    trl = np.stack([edges[:-1], edges[1:], np.zeros(len(lengths))], axis=1)
    return spy.AnalogData(x.astype(np.float32), samplerate=fs, trialdefinition=trl)


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def _compare(data, what, **kw):
    got = _quiet(spy.resampledata, data, **kw)
    ref = _quiet(spy.resampledata, data, **kw, **HOW)
    assert got.data.dtype == np.float32 and got.data.shape == ref.data.shape, what
    assert np.array_equal(np.asarray(got.trialdefinition), np.asarray(ref.trialdefinition)), what
    assert list(got.channel) == list(ref.channel) and got.samplerate == ref.samplerate, what
    worst = max(excess(g, r) for g, r in zip(got.trials, ref.trials))
    print(f"{what}: err/tol {worst:.3g}")
    assert worst <= 1.0, f"{what}: err/tol {worst:.3g}"
    return got, ref


@pytest.mark.parametrize("name,fs,new_fs,order,lpfreq", [c for c in golden_cases() if not c[0].startswith("d")])
def test_ratio_table_at_70_channels_and_recorded_reference(name, fs, new_fs, order, lpfreq):
    n = G[f"{name}_in"].shape[0]
    _compare(_data([n, n], 70, seed=n, fs=fs), name, resamplefs=new_fs, order=order, lpfreq=lpfreq)
    got = _quiet(spy.resampledata, spy.AnalogData(G[f"{name}_in"].copy(), samplerate=fs), resamplefs=new_fs, order=order,
                 lpfreq=lpfreq)
    e = excess(got.data, G[f"{name}_out"])
    print(f"{name} against the recorded reference: err/tol {e:.3g}")
    assert e <= 1.0


def test_recorded_downsample():
    for name, fs, new_fs, _, _ in golden_cases():
        if name.startswith("d"):
            got = spy.resampledata(spy.AnalogData(G[f"{name}_in"].copy(), samplerate=fs), resamplefs=new_fs, method="downsample")
            assert np.array_equal(got.data, G[f"{name}_out"])


# the tiles: 8 outputs per lane and phase (4 for down in 19 ... 42, 1 beyond), 64 channels, chunks of 128 taps per phase.
# 1000 -> 600 has 3 phases: 24 outputs fill one block of each (40 samples); 128 taps per phase are orders 381 ... 383
@pytest.mark.parametrize("nsamp", [39, 40, 41, 80, 82])
@pytest.mark.parametrize("nchan", [1, 63, 64, 65])
def test_tile_boundaries(nsamp, nchan):
    data = _data([nsamp, nsamp], nchan, seed=nsamp + nchan)
    for order in (380, 382, 384, 386, 766, 768):
        _compare(data, f"n={nsamp} c={nchan} order={order}", resamplefs=600, order=order)


@pytest.mark.parametrize("fs,new_fs", [(18000, 1000), (19000, 1000), (42000, 1000), (43000, 1000)])
def test_tile_choice_by_step(fs, new_fs):
    data = _data([2000, 2000, 1999], 65, seed=fs // 1000, fs=float(fs))
    _compare(data, f"{fs} -> {new_fs}", resamplefs=new_fs, order=300)
    _compare(data, f"{fs} -> {new_fs} downsample", resamplefs=new_fs, method="downsample", lpfreq=400, order=300)


@pytest.mark.parametrize("fs,new_fs", [(1000, 600), (30000, 1000)])
def test_order_1000_on_4096(fs, new_fs):
    _compare(_data([4096, 4096], 70, seed=6, fs=float(fs)), f"order 1000 {fs} -> {new_fs}", resamplefs=new_fs, order=1000)


def test_downsample_with_and_without_lpfreq():
    data = _data([1000, 999, 1000, 130], 70, seed=7)
    got = spy.resampledata(data, resamplefs=250, method="downsample")
    for g, x in zip(got.trials, data.trials):
        assert np.array_equal(g, x[::4])
    _compare(data, "downsample", resamplefs=250, method="downsample")
    got, _ = _compare(data, "downsample lpfreq", resamplefs=250, method="downsample", lpfreq=125, order=100)
    filt = spy.preprocessing(data, filter_class="firws", filter_type="lp", freq=125, order=100, direction="twopass")
    same = True
    for g, f in zip(got.trials, filt.trials):
        assert_parity(g, np.asarray(f)[::4], what="decimating second pass against fir_same")
        same = same and np.array_equal(g, np.asarray(f)[::4])
    print(f"downsample lpfreq: bit-identical to preprocessing(firws lp twopass)[::4]: {same}")


def test_unequal_lengths_selection_and_chunks(monkeypatch):
    import importlib
    mod = importlib.import_module("syncopy_amd.preproc.resampledata")
    data = _data([500, 300, 500, 301, 300, 500], 70, seed=10)
    sel = {"trials": [4, 0, 2, 1], "channel": [3, 1, 60], "latency": [0.05, 0.28]}
    for kw in (dict(resamplefs=600, order=200), dict(resamplefs=250, method="downsample", lpfreq=100, order=120),
               dict(resamplefs=200, method="downsample")):
        full = _quiet(spy.resampledata, data, **kw)
        _compare(data, f"unequal {kw}", **kw)
        _compare(data, f"select {kw}", select=sel, **kw)
        monkeypatch.setattr(mod, "CHUNK_BYTES", 500 * 70 * 4)          # one trial per launch
        small = _quiet(spy.resampledata, data, **kw)
        monkeypatch.undo()
        assert np.array_equal(full.data, small.data), kw


@pytest.mark.parametrize("kw,up,down", [(dict(resamplefs=600, order=120), 3, 5),
                                        (dict(resamplefs=250, method="downsample", lpfreq=100, order=40), 1, 4)])
def test_nan_in_one_channel_of_one_trial(kw, up, down):
    data = _data([400, 400, 400], 9, seed=11)
    row = 123
    data.data[400 + row, 4] = np.nan
    data.invalidate()
    got = _quiet(spy.resampledata, data, **kw)
    ref = _quiet(spy.resampledata, data, **kw, **HOW)
    assert got.data.shape == ref.data.shape
    others = [c for c in range(9) if c != 4]
    for t, (g, r) in enumerate(zip(got.trials, ref.trials)):
        if t != 1:
            assert not np.isnan(g).any()
            assert_parity(g, r, what=f"trial {t}")
            continue
        assert not np.isnan(g[:, others]).any()
        assert_parity(g[:, others], r[:, others], what="other channels")
        half = kw["order"] // 2                                  # (ntaps - 1) // 2 of the even order
        if up == 1:
            half *= 2                                            # two passes of the filter ahead of the slicing
        m = np.arange(g.shape[0])
        far = np.abs(m * down - row * up) > half + 2 * down
        assert far.sum() > 0 and np.isfinite(g[far, 4]).all() and np.isfinite(r[far, 4]).all()
        assert_parity(g[far, 4], r[far, 4], what="outside the reach of the NaN")


def test_device_resident_input_and_freqanalysis_chain():
    from oracle_routines import ORACLE_FREQ
    data = _data([1000] * 5, 16, seed=12)
    host = spy.resampledata(data, resamplefs=600)
    data.device_data()
    keep = data._data
    data._data = None                                   # the host array is out of reach: only the device copy can serve
    data.set_pending(lambda: (_ for _ in ()).throw(AssertionError("host copy read")), keep.shape, keep.dtype)
    dev = spy.resampledata(data, resamplefs=600)
    assert np.array_equal(dev.data, host.data)
    res = spy.resampledata(_data([1000] * 5, 16, seed=12), resamplefs=600)
    assert res._device is not None and res._data is None
    spec = spy.freqanalysis(res, method="mtmfft", tapsmofrq=3)
    ref_r = spy.resampledata(_data([1000] * 5, 16, seed=12), resamplefs=600, **HOW)
    ref = spy.freqanalysis(ref_r, method="mtmfft", tapsmofrq=3, compute_method="sequential", routine_classes=ORACLE_FREQ)
    assert_parity(spec.data, ref.data, what="resampledata -> mtmfft")


def test_abi_wrapper_directly():
    import torch
    from syncopy_amd import backend
    from syncopy_amd.preproc import design
    rng = np.random.default_rng(13)
    x = rng.normal(size=(3, 300, 10)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    taps = design.windowed_sinc("hamming", 500, 0.1) * 3                    # 501 taps on 300 samples
    out = backend.upfirdn(xd, torch.empty((3, 180, 10), dtype=torch.float32, device="cuda"), torch.from_numpy(taps).cuda(),
                          3, 5).cpu().numpy()
    for t in range(3):
        assert_parity(out[t], RO.resample64(x[t], taps, 3, 5), what="upfirdn")
    one = torch.ones(1, dtype=torch.float64, device="cuda")
    out = backend.upfirdn(xd, torch.empty((3, 43, 10), dtype=torch.float32, device="cuda"), one, 1, 7).cpu().numpy()
    assert np.array_equal(out, x[:, ::7])
    with pytest.raises(backend.SpyHipError):
        backend.upfirdn(xd, torch.empty((3, 43, 10), dtype=torch.float32, device="cuda"), one, 0, 7)
