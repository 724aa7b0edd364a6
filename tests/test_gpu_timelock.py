"""spy.timelockanalysis on the device (csrc/cov.hip and the trial kernels of csrc/stats.hip) against the NumPy model
(timelock_oracle.py) run through the same front end.

`avg` and `var` are compared bit for bit with spy.mean / spy.var over the trials.  `cov` is held to two bounds: the
project's parity criterion, and element-wise 2^-23 |ref| + 1e-9 sqrt(ref_ii ref_jj) - one float32 rounding plus 1000 times
the float64 dot-product error bound at these lengths.  The parity criterion alone cannot tell a float64 accumulation from
a float32 one (on the CPU, float32 accumulation sits at 0.02 ... 0.05 of its tolerance); the second bound can (float32
accumulation exceeds it 5 ... 18 times).

The second half of the file calls backend.cov itself at the edges of its tiling (csrc/cov_kernel.h: 16 x 16 tiles in
64 x 64 blocks, chunks of COV_KC = 32 rows of which a matrix instruction takes 4, MAX_Z = 65535 trials per launch).

Measured on an MI355X (tools/timelock_bench.py): see DESIGN.md section 8."""
import importlib

import numpy as np
import pytest

import syncopy_amd as spy
import timelock_oracle as TO
from parity import assert_parity
from test_timelock import assert_cov

pytestmark = pytest.mark.gpu
HOW = dict(compute_method="sequential", routine_classes=TO.TIMELOCK_OPS)


def _batch(ntrials, n, nchan, seed=0, dc=0.0):
    """(ntrials, n, nchan) float32: channel scales from 1e-2 to 1e2, correlated channels, a mean of its own per channel
    and trial - a transposed or shifted tile of the covariance cannot pass"""
    rng = np.random.default_rng(seed)
    mix = rng.normal(size=(nchan, nchan)) / np.sqrt(nchan) + np.eye(nchan)
    x = rng.normal(size=(ntrials, n, nchan)) @ mix
    x = x * np.logspace(-2, 2, nchan)[rng.permutation(nchan)] + rng.normal(size=(ntrials, 1, nchan)) + dc
    return x.astype(np.float32)


def _data(ntrials, n, nchan, seed=0, dc=0.0, fs=1000.0, offset=-100):
    e = np.arange(ntrials + 1) * n
    trl = np.stack([e[:-1], e[1:], np.full(ntrials, float(offset))], axis=1)
    return spy.AnalogData(_batch(ntrials, n, nchan, seed, dc).reshape(ntrials * n, nchan), samplerate=fs, trialdefinition=trl)


def _device_cov(x, ddof=None):
    import torch
    from syncopy_amd import backend
    return backend.cov(torch.from_numpy(x).cuda(), ddof=ddof).cpu().numpy()


def _check_cov(x, ddof, what):
    got = _device_cov(x, ddof)
    ref = np.stack([TO.cov(t, ddof) for t in x])
    assert_cov(got, ref, what=what)
    assert np.array_equal(got, got.transpose(0, 2, 1), equal_nan=True), f"{what}: symmetry"
    return got, ref


def _compare(data, what, **kw):
    got = spy.timelockanalysis(data, **kw)
    ref = spy.timelockanalysis(data, **kw, **HOW)
    assert isinstance(got, spy.TimeLockData)
    assert got.data.dtype == np.float32 and np.array_equal(got.data, ref.data, equal_nan=True), what
    assert np.array_equal(got.trialdefinition, ref.trialdefinition) and list(got.channel) == list(ref.channel), what
    assert got.avg.dtype == got.var.dtype == np.float32
    assert np.array_equal(got.avg, ref.avg, equal_nan=True), f"{what}: avg"
    assert np.array_equal(got.var, ref.var, equal_nan=True), f"{what}: var"
    if ref.cov is None:
        assert got.cov is None
    elif kw.get("keeptrials"):
        nchan = len(ref.channel)
        assert got.cov.shape == ref.cov.shape
        assert_cov(got.cov.reshape(-1, nchan, nchan), ref.cov.reshape(-1, nchan, nchan), what=what)
    else:
        assert got.cov.shape == ref.cov.shape and got.cov.dtype == np.float32
        assert_parity(got.cov, ref.cov, what=what)
    return got, ref


@pytest.mark.parametrize("n", [257, 4096])
@pytest.mark.parametrize("nchan", [1, 5, 70, 256])
def test_cov_per_trial_against_the_model(nchan, n):
    data = _data(3, n, nchan, seed=nchan + n)
    for ddof in (None, 0, 3):
        got, _ = _compare(data, f"c={nchan} n={n} ddof={ddof}", covariance=True, keeptrials=True, ddof=ddof)
        assert got.cov.shape == ((3, nchan, nchan) if nchan > 1 else (3,))
        per = got.cov.reshape(3, nchan, nchan)
        assert np.array_equal(per, per.transpose(0, 2, 1))


def test_cov_with_a_dc_offset_of_1e4():
    _compare(_data(3, 4096, 70, seed=1, dc=1e4), "DC offset 1e4", covariance=True, keeptrials=True)


def test_avg_and_var_are_spy_mean_and_spy_var():
    data = _data(7, 300, 33, seed=2)
    sel = {"trials": [5, 0, 3], "channel": [30, 2, 11], "latency": [-0.05, 0.1]}
    for select in (None, sel):
        if select is None:
            tld = spy.timelockanalysis(data)
        else:                                           # the window goes in as `latency`, the rest as the selection
            tld = spy.timelockanalysis(data, latency=sel["latency"], select={"trials": sel["trials"], "channel": sel["channel"]})
        assert np.array_equal(tld.avg, spy.mean(data, dim="trials", select=select).data)
        assert np.array_equal(tld.var, spy.var(data, dim="trials", select=select).data)
        assert data.selection is None


def test_two_runs_give_the_same_bits():
    data = _data(5, 4096, 256, seed=3)
    a = spy.timelockanalysis(data, covariance=True, keeptrials=True)
    b = spy.timelockanalysis(data, covariance=True, keeptrials=True)
    assert np.array_equal(a.cov, b.cov) and np.array_equal(a.avg, b.avg) and np.array_equal(a.var, b.var)
    c = spy.timelockanalysis(data, covariance=True)
    d = spy.timelockanalysis(data, covariance=True)
    assert np.array_equal(c.cov, d.cov)


def test_nan_stays_in_its_row_and_column():
    data = _data(3, 500, 70, seed=4)
    data.data[500 + 17, 66] = np.nan
    data.data[1000, 3] = np.nan
    data.data[1499, 64] = np.nan
    data.invalidate()
    got, ref = _compare(data, "NaN", covariance=True, keeptrials=True)
    assert np.array_equal(np.isnan(got.cov), np.isnan(ref.cov))
    for t, bad in ((0, []), (1, [66]), (2, [3, 64])):
        mask = np.zeros((70, 70), dtype=bool)
        mask[bad, :] = True
        mask[:, bad] = True
        assert np.array_equal(np.isnan(got.cov[t]), mask), t


def test_selection_with_reordered_trials_and_channels_plus_latency():
    data = _data(6, 600, 70, seed=5)
    sel = {"trials": [4, 0, 2, 1], "channel": [3, 69, 1, 60]}
    for keep in (True, False):
        got, _ = _compare(data, f"select keeptrials={keep}", select=sel, latency=[0.0, 0.3], covariance=True, keeptrials=keep)
        assert got.avg.shape == (301, 4) and list(got.channel) == list(data.channel[[3, 69, 1, 60]])
    data.selectdata({"channel": [5, 6]})
    prior = data.selection
    _compare(data, "prior selection", trials=[5, 3], latency="poststim", covariance=True, keeptrials=True)
    assert data.selection is prior


def test_keeptrials_false_against_the_model():
    for nchan, n in ((70, 257), (256, 4096)):
        _compare(_data(9, n, nchan, seed=6 + nchan), f"average c={nchan} n={n}", covariance=True)
    one = _compare(_data(1, 257, 1, seed=7), "one trial, one channel", covariance=True)[0]
    assert one.cov.shape == ()


def test_more_trials_than_fit_one_chunk(monkeypatch):
    mod = importlib.import_module("syncopy_amd.statistics.timelockanalysis")
    data = _data(7, 400, 70, seed=8)
    sel = {"trials": [6, 1, 3, 0, 2], "channel": list(range(69, -1, -3))}
    for kw in (dict(covariance=True), dict(covariance=True, keeptrials=True), dict(covariance=True, select=sel)):
        full = spy.timelockanalysis(data, **kw)
        monkeypatch.setattr(mod, "CHUNK_BYTES", 2 * 400 * 70 * 4)          # two trials per chunk
        small = spy.timelockanalysis(data, **kw)
        monkeypatch.setattr(mod, "CHUNK_BYTES", 1)                         # one trial per chunk
        single = spy.timelockanalysis(data, **kw)
        monkeypatch.undo()
        for name in ("avg", "var", "cov", "data"):
            assert np.array_equal(getattr(full, name), getattr(small, name)), (kw, name)
            assert np.array_equal(getattr(full, name), getattr(single, name)), (kw, name)
    _compare(data, "chunked", covariance=True)


def test_resident_input_is_not_uploaded_again():
    import torch
    data = _data(16, 4096, 256, seed=9)                 # 64 MiB
    host = spy.timelockanalysis(data, covariance=True, keeptrials=True)
    data.device_data()
    torch.cuda.synchronize()
    keep = data._data
    data._data = None                                   # the host array is out of reach: only the device copy can serve
    data.set_pending(lambda: (_ for _ in ()).throw(AssertionError("host copy read")), keep.shape, keep.dtype)
    nbytes = keep.nbytes
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dev = spy.timelockanalysis(data, covariance=True, keeptrials=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"resident: peak device memory grew by {grown} bytes for {nbytes} bytes of data")
    assert grown < nbytes // 2                          # accumulators and results, never another copy of the data
    assert torch.cuda.memory_allocated() - before < nbytes // 2
    for name in ("avg", "var", "cov"):
        assert np.array_equal(getattr(dev, name), getattr(host, name)), name
    assert dev._data is None and np.array_equal(dev.data, keep)     # fetched from the device on first use


def test_abi_wrapper_directly():
    import torch
    from syncopy_amd import backend
    rng = np.random.default_rng(10)
    x = rng.normal(size=(3, 300, 10)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = backend.cov(xd).cpu().numpy()
    for t in range(3):
        assert_cov(out[t], TO.cov(x[t]), what="backend.cov")
    out = backend.cov(xd, ddof=0).cpu().numpy()
    assert_cov(out[1], TO.cov(x[1], 0), what="backend.cov ddof 0")
    with pytest.raises(backend.SpyHipError):
        backend.cov(xd, ddof=300)
    with pytest.raises(backend.SpyHipError):
        backend.cov(xd, ddof=-1)
    from syncopy_amd import abi
    dev = abi.Device(0)
    try:
        assert np.array_equal(dev.cov(x), backend.cov(xd).cpu().numpy())
    finally:
        dev.close()


# ---- backend.cov at tile, block and chunk edges --------------------------------------------------------------------
# tile edges 15/16/17, 31/32/33, 47/48/49; block edges 63/64/65, 127/128/129; 129 channels are three block rows, the
# last with one channel, 257 and 300 five (the walk from the block index to (bi, bj) goes up to bi = 4)
@pytest.mark.parametrize("nchan", [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 257, 300])
def test_cov_channel_counts_at_tile_and_block_edges(nchan):
    _check_cov(_batch(2, 65, nchan, seed=nchan), None, f"backend.cov c={nchan} n=65")


# shorter than one chunk of 32 rows, at it and next to it, two chunks; 2, 3, 5: zero-filled rows in a matrix instruction
@pytest.mark.parametrize("n", [2, 3, 4, 5, 31, 32, 33, 63, 64, 65])
def test_cov_trial_lengths_at_chunk_edges(n):
    x = _batch(2, n, 70, seed=n)
    for ddof in sorted({0, 1, n - 1}):
        _check_cov(x, ddof, f"backend.cov c=70 n={n} ddof={ddof}")


def test_cov_of_one_sample_is_zero():
    got = _device_cov(_batch(2, 1, 70, seed=1), ddof=0)
    assert got.shape == (2, 70, 70) and not got.any() and not np.signbit(got).any()


def test_cov_65537_trials_second_launch():
    """MAX_Z = 65535 trials go into one launch: trials 65535 and 65536 are the second one's, which offsets x and out"""
    x = _batch(65537, 2, 3, seed=65537)
    got = _device_cov(x)
    d = x.astype(np.float64) - x.astype(np.float64).mean(axis=1, keepdims=True)
    ref = np.einsum("tki,tkj->tij", d, d).astype(np.float32)               # n - ddof = 1
    assert_cov(got, ref, what="65537 trials")
    assert np.array_equal(got, got.transpose(0, 2, 1))
    for t in (0, 65534, 65535, 65536):
        assert_cov(got[t], TO.cov(x[t]), what=f"trial {t} of 65537")


def test_cov_nan_across_a_block_edge():
    x = _batch(3, 65, 130, seed=130)
    x[0, 7, 63] = np.nan
    x[1, 64, 64] = np.nan
    x[2, 0, 63] = x[2, 33, 64] = np.nan
    got, _ = _check_cov(x, None, "NaN in channels 63 and 64")
    for t, bad in ((0, [63]), (1, [64]), (2, [63, 64])):
        mask = np.zeros((130, 130), dtype=bool)
        mask[bad, :] = True
        mask[:, bad] = True
        assert np.array_equal(np.isnan(got[t]), mask), t
