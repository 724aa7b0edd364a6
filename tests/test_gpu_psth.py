"""spy.spike_psth on the device: the kernels of syncopy_amd/csrc/psth_kernel.h through the front end, through the tensor
wrappers and once through the NumPy + ctypes host, against the NumPy model (tests/psth_oracle.py) and the results recorded
from the reference (tests/golden/psth.npz), at the smallest shapes that reach every dispatch edge.

Criteria, as in tests/test_psth.py: spikecount and rate bit for bit, proportion within 2 float32 ulp with identical NaN
positions.  Timing (tools/psth_bench.py): see DESIGN.md section 8."""
import numpy as np
import pytest

import psth_drive as D
import psth_oracle as PO
import syncopy_amd as spy
from syncopy_amd.shared.trial_chunks import applied_selection
from syncopy_amd.statistics import spike_psth as SP

pytestmark = pytest.mark.gpu


def check(data, select=None, outputs=D.OUTPUTS, **kw):
    """spy.spike_psth against the model for every output; returns the last result and its host-side plan"""
    for output in outputs:
        tld = spy.spike_psth(data, output=output, select=select, **kw)
        with applied_selection(data, select):
            plan = SP._plan(data, kw.get("binsize", "rice"), output, kw.get("latency", "maxperiod"),
                            kw.get("vartriallen", True))
        cols, ref = D.oracle_for(data, plan, select)
        assert tld.channel.tolist() == [f"channel{c}_unit{u}" for c, u in cols]
        assert np.array_equal(tld.info["bins"], plan.edges) and tld.info["numDiscard"] == plan.numDiscard
        assert np.array_equal(tld.trialdefinition, plan.trialdefinition) and tld.samplerate == plan.out_samplerate
        PO.assert_psth(tld.data, ref, output, output)
    return tld, plan


def device_histogram(table, k):
    """the kernels through the tensor wrappers of backend.py for kernel inputs `k` (psth_drive.inputs_from_columns)"""
    import torch
    from syncopy_amd import backend
    table = np.asarray(table, dtype=np.int64)
    up = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()      # noqa: E731
    sample, chan, unit = up(table[:, 0]), up(table[:, 1], np.int32), up(table[:, 2], np.int32)
    row_lo, row_hi, edges, lut = up(k.row_lo), up(k.row_hi), up(k.edges), up(k.lut)
    rows = backend.psth_bin_rows(sample, row_lo, row_hi, up(k.start), up(k.onset), edges, k.samplerate)
    out = backend.psth_count(chan, unit, rows, lut, k.C, k.U, up(k.lohi), k.ncols, k.scale)
    if k.output == "proportion":
        backend.psth_proportion(chan, unit, row_lo, row_hi, rows, lut, k.C, k.U, up(k.unit_k), up(k.col_k), k.nk, edges,
                                out)
    return out.cpu().numpy().reshape(-1, k.ncols)


@pytest.mark.parametrize("name", D.golden_names())
def test_kernels_match_reference(name):
    tab, par, edges, cols = D.golden_case(name)
    for output in D.OUTPUTS:
        k = D.inputs_from_columns(tab, [[par[0], par[1], par[2]]], edges, output, par[3], cols)
        PO.assert_psth(device_histogram(tab, k), D.golden()[f"{name}_{output}"], output, f"{name} {output}")


def test_front_end_matches_reference():
    # the recorded case whose edges the front end rebuilds to the bit: np.arange over the trial's own window
    tab, par, edges, cols = D.golden_case("arange_24k")
    data = spy.SpikeData(tab, samplerate=par[3], trialdefinition=[par[:3]])
    w0, w1 = par[2] / par[3], (par[1] - par[0] - 1 + par[2]) / par[3]
    for output in D.OUTPUTS:
        tld = spy.spike_psth(data, binsize=0.0137, latency=[w0, w1], output=output)
        assert np.array_equal(tld.info["bins"], edges)
        assert tld.channel.tolist() == [f"channel{c}_unit{u}" for c, u in cols]
        PO.assert_psth(tld.data, D.golden()[f"arange_24k_{output}"], output, output)


def test_numpy_host():
    from syncopy_amd import abi
    data = D.make_data([(500, -100), (450, -50), (500, -120)], per_trial=[200, 0, 150], between=5, seed=21)
    edges = np.arange(-0.15, 0.45 + 0.04, 0.04)
    dev = abi.Device(0)
    try:
        for output in D.OUTPUTS:
            got, cols = dev.psth(data.data, data.trialdefinition, data.samplerate, edges, output=output, channels=[0, 2])
            want_cols, ref = PO.psth(data.data, data.trialdefinition, [0, 1, 2], edges, output, data.samplerate, [0, 2])
            assert np.array_equal(cols, want_cols) and got.shape == (3, len(edges) - 1, len(cols))
            PO.assert_psth(got.reshape(-1, len(cols)), ref, output, output)
    finally:
        dev.close()


def test_one_trial_one_column_one_bin():
    data = spy.SpikeData([[3, 0, 0], [5, 0, 0], [9, 0, 0]], samplerate=10.0, trialdefinition=[[0, 10, 0]])
    tld, plan = check(data, binsize=0.9, latency=[0.0, 0.9])
    assert tld.data.shape == (1, 1) and plan.nbins == 1


@pytest.mark.parametrize("nbins", [D.BIN_TILE - 1, D.BIN_TILE, D.BIN_TILE + 1])
def test_bins_at_the_tile(nbins):
    data = D.make_data([(640, -64), (600, -40), (640, -64)], per_trial=150, seed=nbins)
    _, plan = check(data, binsize=0.015625, latency=[-0.0625, -0.0625 + nbins * 0.015625 - 0.001])
    assert plan.nbins == nbins


@pytest.mark.parametrize("ncols", [D.COL_TILE - 1, D.COL_TILE, D.COL_TILE + 1])
def test_columns_at_the_tile(ncols):
    pairs = [(c, u) for c in range(13) for u in range(10)][:ncols]
    data = D.make_data([(500, -100), (450, -50), (500, 0)], per_trial=400, seed=ncols, pairs=pairs)
    _, plan = check(data, binsize=0.1)
    assert plan.ncols == ncols


def test_a_bin_with_more_spikes_than_threads():
    data = D.make_data([(300, 0), (300, 0)], per_trial=[3 * D.THREADS + 7, 5], nchan=2, nunit=2, seed=5)
    check(data, binsize=0.15)


def test_empty_trials_gaps_and_equal_samples():
    data = D.make_data([(400, -100), (400, -100), (400, 500), (400, -100)], per_trial=[80, 0, 40, 90], between=6, seed=9)
    tab = data.data.copy()
    own = data.trial_rows[3]
    tab[own[0]:own[1], 0] = tab[own[0], 0] + (np.arange(own[1] - own[0]) // 30) * 100
    data = spy.SpikeData(tab, samplerate=1000.0, trialdefinition=data.trialdefinition)
    assert (data.trialid == -1).sum() == 24 and len(data.trials[1]) == 0
    tld, plan = check(data, binsize=0.05, latency=[-0.1, 0.25])
    nb = plan.nbins
    assert np.isnan(tld.data[2 * nb:3 * nb]).all() and not np.isnan(tld.data[nb:2 * nb]).any()


def test_many_trials_on_the_grid():
    # 65537 trials of one or two spikes, 2 bins, 1 column: past a 16-bit grid dimension
    T, n = 65537, 10
    rng = np.random.default_rng(8)
    first = np.arange(T) * n + rng.integers(0, n, size=T)
    second = (np.arange(T) * n + rng.integers(0, n, size=T))[::2]
    samples = np.sort(np.concatenate([first, second]))
    tab = np.stack([samples, np.zeros_like(samples), np.zeros_like(samples)], axis=1)
    trl = np.stack([np.arange(T) * n, np.arange(T) * n + n, np.zeros(T)], axis=1)
    data = spy.SpikeData(tab, samplerate=10.0, trialdefinition=trl)
    tld = spy.spike_psth(data, binsize=0.45, latency=[0.0, 0.9], output="spikecount")
    edges = np.arange(0.0, 0.9 + 0.45, 0.45)
    assert np.array_equal(tld.info["bins"], edges) and tld.data.shape == (2 * T, 1)
    t = (samples % n) / 10.0
    want = np.zeros((T, 2), dtype=np.float32)
    np.add.at(want, (samples // n, np.where(t < edges[1], 0, 1)), 1)
    assert np.array_equal(tld.data.reshape(T, 2), want) and want.sum() == samples.size
    assert np.array_equal(tld.avg.ravel(), spy.mean(_as_analog(tld), dim="trials").data.ravel())


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("fs", [30000.0, 24414.0625])
def test_samples_above_2_31_and_edge_adversary(fs, exact):
    data, window, binsize = D.edge_adversary(fs, exact)
    assert data.data[0, 0] > 2 ** 31
    check(data, binsize=binsize, latency=window)


def test_selections():
    data = D.make_data([(500, -100)] * 4, per_trial=120, nchan=4, nunit=5, seed=3)
    tld, plan = check(data, binsize=0.1, select={"trials": [3, 1, 1, 0], "channel": [0, 2], "unit": ["unit2", "unit5"]})
    assert plan.trial_ids == [3, 1, 1, 0] and tld.channel.tolist() == ["channel0_unit1", "channel0_unit4",
                                                                       "channel2_unit1", "channel2_unit4"]
    nb = plan.nbins
    assert np.array_equal(tld.data[nb:2 * nb], tld.data[2 * nb:3 * nb], equal_nan=True)
    assert data.selection is None
    check(data, binsize=0.1, select={"channel": slice(1, 3), "unit": slice(None, None, 2)})
    check(data, binsize=0.1, latency=[-0.1, 0.3], vartriallen=False, select={"trials": [2, 0]})


def _as_analog(tld):
    return spy.AnalogData(tld.data, samplerate=tld.samplerate, trialdefinition=tld.trialdefinition)


@pytest.mark.parametrize("output", D.OUTPUTS)
def test_keeptrials_both_ways_and_trial_moments(output):
    data = D.make_data([(500, -100), (420, -60), (480, -120), (500, -100)], per_trial=300, seed=11)
    kept = spy.spike_psth(data, binsize=0.05, output=output)
    assert np.isnan(kept.data).any()                              # the shorter trials leave NaN bins
    ad = _as_analog(kept)
    assert np.array_equal(kept.avg, spy.mean(ad, dim="trials").data, equal_nan=True)
    assert np.array_equal(kept.var, spy.var(ad, dim="trials").data, equal_nan=True)
    assert np.array_equal(np.isnan(kept.avg), np.isnan(kept.data.reshape(4, -1, kept.data.shape[1])).any(axis=0))
    avg = spy.spike_psth(data, binsize=0.05, output=output, keeptrials=False)
    assert avg.data is None and avg.trialdefinition.shape == (1, 3)
    assert np.array_equal(avg.trialdefinition, kept.trialdefinition[:1])
    assert np.array_equal(avg.avg, kept.avg, equal_nan=True) and np.array_equal(avg.var, kept.var, equal_nan=True)
    assert avg.cfg["spike_psth"]["keeptrials"] is False and avg.cfg["spike_psth"]["output"] == output


def test_two_calls_give_the_same_bits_and_the_upload_is_kept():
    data = spy.synthdata.poisson_noise(nTrials=20, nSpikes=20000, seed=5)
    cols = data.device_columns()
    assert [c.dtype for c in cols] == [__import__("torch").int64, __import__("torch").int32, __import__("torch").int32]
    for output in D.OUTPUTS:
        a = spy.spike_psth(data, output=output)
        b = spy.spike_psth(data, output=output)
        assert a.data.tobytes() == b.data.tobytes() and a.avg.tobytes() == b.avg.tobytes()
    assert data.device_columns()[0] is cols[0]
    data.invalidate()
    assert data.device_columns()[0] is not cols[0]
    check(data, outputs=("rate",), binsize="sqrt", latency="minperiod")


def test_chunks_of_trials(monkeypatch):
    data = D.make_data([(500, -100)] * 7, per_trial=100, seed=13)
    whole = spy.spike_psth(data, binsize=0.05, output="proportion")
    monkeypatch.setattr(SP, "CHUNK_BYTES", 3 * whole.data.shape[1] * (whole.data.shape[0] // 7) * 4)
    parts = spy.spike_psth(data, binsize=0.05, output="proportion")
    for name in ("data", "avg", "var"):
        assert getattr(whole, name).tobytes() == getattr(parts, name).tobytes()
