"""spy.spike_psth without a GPU: the NumPy model against results recorded from the reference (tests/golden/psth.npz,
tools/record_psth_golden.py), a CPU emulation of the kernels of syncopy_amd/csrc/psth_kernel.h against the model at their
dispatch edges, and every rule of the front end above the kernels (`_plan`), SpikeData and poisson_noise.

Criteria: spikecount and rate bit for bit (integer counts, the same float64 product); proportion within 2 float32 ulp with
identical NaN positions (one differing float64 operation order ahead of the single rounding)."""
import ctypes as C

import numpy as np
import pytest

import psth_drive as D
import psth_oracle as PO
import syncopy_amd as spy
from syncopy_amd.shared.errors import SPYError, SPYTypeError, SPYValueError
from syncopy_amd.shared.trial_chunks import applied_selection
from syncopy_amd.statistics import spike_psth as SP


# ---- the model against the reference's recorded results ------------------------------------------------------------
@pytest.mark.parametrize("output", D.OUTPUTS)
@pytest.mark.parametrize("name", D.golden_names())
def test_oracle_matches_reference(name, output):
    tab, par, edges, cols = D.golden_case(name)
    got = PO.trial_psth(tab, par[0], par[1], par[2], [tuple(c) for c in cols], edges, output, par[3])
    PO.assert_psth(got, D.golden()[f"{name}_{output}"], output, f"{name} {output}")


def test_golden_file_holds_the_cases():
    g = D.golden()
    names = set(D.golden_names())
    assert len(names) >= 12
    assert {float(g[f"{n}_par"][3]) for n in names} >= {1000.0, 30000.0, 24414.0625}
    assert np.isnan(g["window_behind_rate"]).all() and np.isnan(g["window_before_rate"]).all()
    head = np.isnan(g["nan_head_tail_spikecount"][:, 0])
    assert head[0] and head[-1] and not head.all()
    assert np.isnan(g["unit_outside_window_proportion"]).any() and not np.isnan(g["unit_outside_window_rate"]).any()
    tab, par, edges, _ = D.golden_case("last_edge")
    assert np.any((tab[:, 0] - par[0] + par[2]) / par[3] == edges[-1])
    for n in names:                                    # all channels 0 .. C-1 in the trial
        ch = g[f"{n}_spikes"][:, 1]
        assert set(ch.tolist()) == set(range(int(ch.max()) + 1)), n


# ---- CPU emulation of psth_kernel.h --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return D.build_emu()


def cpu_psth(emu, data, binsize="rice", output="rate", latency="maxperiod", vartriallen=True, select=None):
    """(plan, stacked result): the front end's _plan, with every kernel emulated"""
    with applied_selection(data, select):
        plan = SP._plan(data, binsize, output, latency, vartriallen, presence=D.emu_presence(emu, data.data))
    return plan, D.emu_histogram(emu, data.data, plan)


def check(emu, data, select=None, outputs=D.OUTPUTS, **kw):
    for output in outputs:
        plan, got = cpu_psth(emu, data, output=output, select=select, **kw)
        cols, ref = D.oracle_for(data, plan, select)
        assert np.array_equal(plan.columns, cols)
        PO.assert_psth(got, ref, output, output)
    return plan


def test_emu_tiles_are_the_headers(emu):
    v = [C.c_int() for _ in range(5)]
    emu.emu_psth_tiles(*[C.byref(x) for x in v])
    assert [x.value for x in v] == [D.BIN_TILE, D.COL_TILE, D.UNIT_TILE, D.PROP_TILE, D.THREADS]


def test_emu_refuses_more_units_with_a_column_than_units(emu):
    z = np.zeros(8, dtype=np.int64)
    args = lambda nk: [emu.ctx] + [D._p(z)] * 6 + [2, 3, D._p(z), D._p(z), nk, D._p(z), 1, 4, 2, D._p(z), D._p(z)]      # noqa: E731
    assert emu.spyhip_psth_proportion(*args(4)) == -1              # nk > nunit = 3
    assert emu.spyhip_psth_proportion(*args(0)) == -1


@pytest.mark.parametrize("name", D.golden_names())
def test_emu_kernels_match_reference(emu, name):
    tab, par, edges, cols = D.golden_case(name)
    for output in D.OUTPUTS:
        k = D.inputs_from_columns(tab, [[par[0], par[1], par[2]]], edges, output, par[3], cols)
        assert np.array_equal(k.columns, cols)
        PO.assert_psth(D.emu_histogram(emu, tab, k), D.golden()[f"{name}_{output}"], output, f"{name} {output}")


def test_emu_one_trial_one_column_one_bin(emu):
    data = spy.SpikeData([[3, 0, 0], [5, 0, 0], [9, 0, 0]], samplerate=10.0, trialdefinition=[[0, 10, 0]])
    plan = check(emu, data, binsize=0.9, latency=[0.0, 0.9])
    assert (plan.nbins, plan.ncols) == (1, 1)


@pytest.mark.parametrize("nbins", [D.BIN_TILE - 1, D.BIN_TILE, D.BIN_TILE + 1])
def test_emu_bins_at_the_tile(emu, nbins):
    data = D.make_data([(640, -64), (600, -40)], per_trial=150, seed=nbins)
    plan = check(emu, data, binsize=0.015625, latency=[-0.0625, -0.0625 + nbins * 0.015625 - 0.001])
    assert plan.nbins == nbins


@pytest.mark.parametrize("ncols", [D.COL_TILE - 1, D.COL_TILE, D.COL_TILE + 1])
def test_emu_columns_at_the_tile(emu, ncols):
    pairs = [(c, u) for c in range(13) for u in range(10)][:ncols]
    data = D.make_data([(500, -100), (450, -50)], per_trial=400, seed=ncols, pairs=pairs)
    plan = check(emu, data, binsize=0.1)
    assert plan.ncols == ncols and plan.nk == 10


def test_emu_a_bin_with_more_spikes_than_threads(emu):
    data = D.make_data([(300, 0), (300, 0)], per_trial=[3 * D.THREADS + 7, 5], nchan=2, nunit=2, seed=5)
    plan = check(emu, data, binsize=0.15)
    assert plan.nbins == 2


def test_emu_empty_trials_gaps_and_equal_samples(emu):
    # a trial without spikes, a trial whose spikes all lie outside the window, spikes between the trials, and a trial of
    # many equal sample numbers
    data = D.make_data([(400, -100), (400, -100), (400, 500), (400, -100)], per_trial=[80, 0, 40, 90], between=6, seed=9)
    tab = data.data.copy()
    own = data.trial_rows[3]
    tab[own[0]:own[1], 0] = tab[own[0], 0] + (np.arange(own[1] - own[0]) // 30) * 100
    data = spy.SpikeData(tab, samplerate=1000.0, trialdefinition=data.trialdefinition)
    assert (data.trialid == -1).sum() == 24 and len(data.trials[1]) == 0
    plan = check(emu, data, binsize=0.05, latency=[-0.1, 0.25])
    assert plan.lohi[2].tolist() == [plan.nbins, plan.nbins]


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("fs", [30000.0, 24414.0625])
def test_emu_samples_above_2_31_and_edge_adversary(emu, fs, exact):
    data, window, binsize = D.edge_adversary(fs, exact)
    assert data.data[0, 0] > 2 ** 31
    plan = check(emu, data, binsize=binsize, latency=window)
    t = (data.data[:, 0] - 3_000_000_000 + plan.onset[0]) / fs
    if exact:
        assert np.sum(t == plan.edges[-1]) >= 2 and np.sum(np.isin(t, plan.edges)) >= 4
    else:
        assert np.sum(np.abs(t[:, None] - plan.edges[None, :]).min(axis=0) < 1e-12) >= plan.nbins // 2


def test_emu_selections(emu):
    data = D.make_data([(500, -100)] * 4, per_trial=120, nchan=4, nunit=5, seed=3)
    plan = check(emu, data, binsize=0.1, select={"trials": [3, 1, 1, 0], "channel": [0, 2], "unit": ["unit2", "unit5"]})
    assert plan.trial_ids == [3, 1, 1, 0] and plan.columns.tolist() == [[0, 1], [0, 4], [2, 1], [2, 4]]
    assert int((plan.lut < 0).sum()) == plan.C * plan.U - 4
    plan = check(emu, data, binsize=0.1, select={"channel": slice(1, 3), "unit": slice(None, None, 2)})
    assert sorted(set(plan.columns[:, 0])) == [1, 2] and sorted(set(plan.columns[:, 1])) == [0, 2, 4]


def test_emu_many_units(emu):
    pairs = [(0, u) for u in range(D.UNIT_TILE + 3)]
    data = D.make_data([(2000, 0)], per_trial=D.UNIT_TILE + 40, pairs=pairs, seed=2)
    plan = check(emu, data, binsize=1.0, outputs=("proportion",))
    assert plan.nk == D.UNIT_TILE + 3


# ---- the front end above the kernels -------------------------------------------------------------------------------
def _data(**kw):
    kw.setdefault("seed", 11)
    return D.make_data([(500, -100), (420, -60), (480, -120), (500, -100)], **kw)


@pytest.mark.parametrize("kw,exc", [
    (dict(output="counts"), SPYValueError), (dict(binsize="scott"), SPYValueError), (dict(binsize=None), SPYTypeError),
    (dict(vartriallen=1), SPYTypeError), (dict(keeptrials="yes"), SPYTypeError), (dict(keeptrials=None), SPYTypeError),
    (dict(foo=1), SPYValueError), (dict(latency="always"), SPYValueError), (dict(latency=[0.1]), SPYValueError),
    (dict(binsize=-0.01), SPYValueError), (dict(binsize=5.0), SPYValueError), (dict(binsize=0), SPYValueError),
    (dict(latency=[5.0, 6.0]), SPYValueError), (dict(latency=[-6.0, -5.0]), SPYValueError),
    (dict(latency=[0.2, 0.1]), SPYValueError),
    (dict(select={"latency": [0, 0.1]}), SPYValueError), (dict(select={"trials": [9]}), SPYValueError),
    (dict(select={"channel": ["channel9"]}), SPYValueError), (dict(select={"unit": [17]}), SPYValueError),
    (dict(select={"frequency": 1}), SPYValueError),
    (dict(latency=[-0.11, 0.4], vartriallen=False), SPYValueError),
])
def test_argument_errors(kw, exc):
    data = _data()
    with pytest.raises(exc):
        spy.spike_psth(data, **kw)
    assert data.selection is None


def test_input_errors():
    with pytest.raises(SPYTypeError):
        spy.spike_psth(np.zeros((4, 3), dtype=int))
    with pytest.raises(SPYTypeError):
        spy.spike_psth(spy.AnalogData(np.zeros((10, 2), dtype=np.float32), samplerate=1.0))
    with pytest.raises(SPYValueError):
        spy.spike_psth(spy.SpikeData())
    with pytest.raises(SPYValueError, match="latency="):
        _data().selectdata({"latency": "maxperiod"})


def test_no_gpu_means_the_usual_error():
    import torch
    from syncopy_amd._lib import SpyHipError
    data = _data()
    if torch.cuda.is_available():
        assert spy.spike_psth(data, parallel=False, chan_per_worker=2).avg.shape[1] == 12
    else:
        with pytest.raises(SpyHipError, match="no HIP device"):
            spy.spike_psth(data, parallel=False, chan_per_worker=2)
    assert data.selection is None


@pytest.mark.parametrize("rule,n", [("rice", lambda m: int(2 * m ** (1 / 3))), ("sqrt", lambda m: int(np.ceil(np.sqrt(m))))])
def test_rules_give_n_edges_from_the_mean_trial_length_in_samples(rule, n):
    data = _data()
    with applied_selection(data, None):
        plan = SP._plan(data, rule, "rate", "maxperiod", True)
    mean_len = (500 + 420 + 480 + 500) / 4                       # samples, not spikes (60 per trial)
    assert len(plan.edges) == n(mean_len) and plan.nbins == n(mean_len) - 1
    assert np.array_equal(plan.edges, np.linspace(-0.12, 0.399, n(mean_len)))
    sub = SP._plan(data.selectdata({"trials": [1, 1, 2]}), rule, "rate", "maxperiod", True)
    assert len(sub.edges) == n((420 + 420 + 480) / 3)
    data.selectdata(None)


def test_numeric_binsize_limits_and_edges():
    data = _data()
    plan = SP._plan(data, 0.05, "rate", [-0.1, 0.3], True)
    assert np.array_equal(plan.edges, np.arange(-0.1, 0.3 + 0.05, 0.05)) and plan.edges.dtype == np.float64
    assert plan.scale == 1 / np.diff(plan.edges)[0]
    assert SP._plan(data, 0.4, "rate", [-0.1, 0.3], True).nbins >= 1                 # the window's width is allowed
    for bad in (0.4000001, -1e-9):
        with pytest.raises(SPYValueError):
            SP._plan(data, bad, "rate", [-0.1, 0.3], True)


def test_latency_words_and_range_errors():
    data = _data()
    iv = data.trialintervals
    assert np.allclose(iv, [[-0.1, 0.399], [-0.06, 0.359], [-0.12, 0.359], [-0.1, 0.399]])
    want = {"maxperiod": [-0.12, 0.399], "minperiod": [-0.06, 0.359], "prestim": [-0.12, 0], "poststim": [0, 0.399]}
    for word, window in want.items():
        assert SP._plan(data, 0.05, "rate", word, True).window == window, word
    sub = data.selectdata({"trials": [1, 2]})
    assert SP._plan(sub, 0.05, "rate", "maxperiod", True).window == [-0.12, 0.359]
    data.selectdata(None)
    assert SP.analysis_window(iv, [0.399, 0.5]) == [0.399, 0.5] and SP.analysis_window(iv, [-1, -0.12]) == [-1.0, -0.12]
    for bad in ([0.3991, 0.5], [-1.0, -0.1201], [0.2, 0.1]):
        with pytest.raises(SPYValueError):
            SP.analysis_window(iv, bad)
    post = D.make_data([(100, 10), (100, 20)])
    with pytest.raises(SPYValueError, match="pre-stimulus"):
        SP._plan(post, 0.01, "rate", "prestim", True)
    pre = D.make_data([(100, -200), (100, -300)])
    with pytest.raises(SPYValueError, match="post-stimulus"):
        SP._plan(pre, 0.01, "rate", "poststim", True)
    apart = D.make_data([(100, 0), (100, 500)])
    with pytest.raises(SPYValueError, match="overlapping"):
        SP._plan(apart, 0.01, "rate", "minperiod", True)


def test_vartriallen_false_discards_in_selection_order(emu):
    data = _data()
    plan = check(emu, data, binsize=0.05, latency=[-0.1, 0.36], vartriallen=False)
    assert plan.trial_ids == [0, 3] and plan.numDiscard == 2 and plan.log_dict["numDiscard"] == 2
    assert not np.isnan(D.emu_histogram(emu, data.data, plan)).any()
    plan = check(emu, data, binsize=0.05, latency=[-0.1, 0.36], vartriallen=False, select={"trials": [3, 2, 0, 3]})
    assert plan.trial_ids == [3, 0, 3] and plan.numDiscard == 1
    assert data.selection is None
    with pytest.raises(SPYValueError, match="covering"):
        SP._plan(data, 0.05, "rate", [-0.12, 0.399], False)
    assert SP._plan(data, 0.05, "rate", [-0.1, 0.36], True).numDiscard == 0


def test_channel_bins_follow_the_intent_not_the_reference(emu):
    # a trial without channel 0: spikes on channels 1, 2, 2 and the columns (0,0), (1,0), (2,0)
    data = spy.SpikeData([[5, 1, 0], [6, 2, 0], [7, 2, 0], [25, 0, 0]], samplerate=10.0,
                         trialdefinition=[[0, 10, 0], [20, 30, 0]])
    plan, got = cpu_psth(emu, data, binsize=0.9, output="spikecount", latency=[0.0, 0.9])
    assert plan.columns.tolist() == [[0, 0], [1, 0], [2, 0]] and plan.labels == ["channel0_unit0", "channel1_unit0",
                                                                                "channel2_unit0"]
    assert got.tolist() == [[0, 1, 2], [1, 0, 0]]
    check(emu, data, binsize=0.9, latency=[0.0, 0.9])


def test_metadata_of_the_result():
    data = _data()
    plan = SP._plan(data, 0.05, "rate", [-0.1, 0.3], True)
    mid = (plan.edges[:-1] + plan.edges[1:]) / 2
    assert plan.out_samplerate == 1 / np.diff(mid).mean() and abs(plan.out_samplerate - 20) < 1e-9
    nb = plan.nbins
    assert np.array_equal(plan.trialdefinition[:, 0], np.arange(4) * nb)
    assert np.array_equal(plan.trialdefinition[:, 1], np.arange(1, 5) * nb)
    assert np.all(plan.trialdefinition[:, 2] == np.rint(mid[0] * plan.out_samplerate))
    assert plan.labels[0] == "channel0_unit0" and plan.labels[-1] == "channel2_unit3" and len(plan.labels) == 12
    assert set(plan.log_dict) == {"bins", "binsize", "latency", "output", "vartriallen", "numDiscard"}
    assert np.array_equal(plan.log_dict["bins"], plan.edges)
    assert plan.lohi.dtype == np.int32 and plan.lohi.shape == (4, 2) and plan.lut.dtype == np.int32


def test_nan_mask_rules():
    edges = np.arange(-0.5, 1.25, 0.25)                          # 7 edges, 6 bins
    # start / end / onset in samples at 1000 Hz: the trial spans [-0.2, 0.8] in time
    assert SP.valid_bins(edges, 100, 1100, -200, 1000.0) == (2, 6)       # head masked up to the first edge >= start
    assert SP.valid_bins(edges, 100, 700, -200, 1000.0) == (2, 4)        # tail from the first edge > end
    assert SP.valid_bins(edges, 0, 2000, -500, 1000.0) == (0, 6)         # index 0: no mask at either end
    assert SP.valid_bins(edges, 0, 100, 2000, 1000.0) == (6, 6)          # all edges before the trial
    assert SP.valid_bins(edges, 0, 100, -900, 1000.0) == (6, 6)          # all edges behind it
    for args in ((100, 1100, -200), (100, 700, -200), (0, 2000, -500), (0, 100, 2000), (0, 100, -900)):
        assert SP.valid_bins(edges, *args, 1000.0) == PO.valid_range(edges, *args, 1000.0)
    # the vectorised form the plan uses, on trials whose ends fall on, just before and just behind edges
    rng = np.random.default_rng(4)
    start = rng.integers(0, 50, size=400)
    end = start + rng.integers(1, 2500, size=400)
    onset = rng.integers(-1500, 1500, size=400)
    onset[:100] = (rng.integers(-2, 5, size=100) * 250) + rng.integers(-1, 2, size=100)
    end[100:200] = start[100:200] - onset[100:200] + rng.integers(-2, 5, size=100) * 250 + rng.integers(-1, 2, size=100)
    end = np.maximum(end, start + 1)
    one = [SP.valid_bins(edges, s, e, o, 1000.0) for s, e, o in zip(start, end, onset)]
    assert SP.valid_bins_all(edges, start, end, onset, 1000.0).tolist() == [list(x) for x in one]
    assert one == [PO.valid_range(edges, s, e, o, 1000.0) for s, e, o in zip(start, end, onset)]


def test_selection_is_restored_and_select_keys():
    data = _data().selectdata({"trials": [2, 0]})
    with pytest.raises(SPYError):                                 # reaches the device, or fails before it
        spy.spike_psth(data, binsize=0.05, select={"trials": [1]}, latency="never")
    assert data.selection.select == {"trials": [2, 0]} and data.selection.trial_ids == [2, 0]
    assert np.array_equal(data.selection.trialdefinition, data.trialdefinition[[2, 0]])
    assert np.allclose(data.selection.trialintervals, data.trialintervals[[2, 0]])
    sel = spy.datatype.SpikeSelection(data, {"channel": "channel2", "unit": [0, 3]})
    assert sel.channel == [1] and sel.unit == [0, 3] and sel.trial_ids == [0, 1, 2, 3]


# ---- SpikeData and poisson_noise -----------------------------------------------------------------------------------
def test_spikedata_sorts_and_converts():
    raw = np.array([[30, 1, 0], [10, 0, 2], [30, 0, 1], [20, 2, 2]], dtype=np.int16)
    d = spy.SpikeData(raw, samplerate=100.0, trialdefinition=[[0, 25, -5], [28, 40, 0]])
    assert d.data.dtype == np.int64 and d.data.tolist() == [[10, 0, 2], [20, 2, 2], [30, 1, 0], [30, 0, 1]]   # stable
    assert d.dimord == ["sample", "channel", "unit"]
    assert d.trial_rows.tolist() == [[0, 2], [2, 4]] and d.trialid.tolist() == [0, 0, 1, 1]
    assert [t.tolist() for t in d.time] == [[0.05, 0.15], [0.02, 0.02]]
    assert np.allclose(d.trialintervals, [[-0.05, 0.19], [0.0, 0.11]])
    assert d.sampleinfo.tolist() == [[0, 25], [28, 40]] and [len(t) for t in d.trials] == [2, 2]
    assert d.channel.tolist() == ["channel1", "channel2", "channel3"] and d.unit.tolist() == ["unit1", "unit2", "unit3"]
    f = spy.SpikeData(raw.astype(np.float64), samplerate=100.0)
    assert f.data.dtype == np.int64 and f.trialdefinition.tolist() == [[10, 30, 0]]
    p = spy.SpikeData(raw[:, [2, 0, 1]], samplerate=100.0, dimord=["unit", "sample", "channel"])
    assert np.array_equal(p.data, d.data) and p.dimord == ["sample", "channel", "unit"]
    wide = spy.SpikeData([[5, 0, 0], [7, 11, 104]], samplerate=1.0)
    assert wide.channel.tolist() == ["channel01", "channel12"] and wide.unit.tolist() == ["unit001", "unit105"]


def test_spikedata_trialid_between_trials():
    tab = np.stack([np.arange(0, 100, 5), np.zeros(20, int), np.zeros(20, int)], axis=1)
    d = spy.SpikeData(tab, samplerate=10.0, trialdefinition=[[10, 30, 0], [50, 70, 0]])
    want = np.full(20, -1)
    want[2:6], want[10:14] = 0, 1
    assert d.trialid.tolist() == want.tolist()


@pytest.mark.parametrize("bad,exc", [
    (np.array([[1, -1, 0]]), SPYValueError), (np.array([[1, 0, -2]]), SPYValueError),
    (np.array([[1, 2 ** 31, 0]]), SPYValueError), (np.array([[1, 0, 2 ** 31]]), SPYValueError),
    (np.array([[1.5, 0, 0]]), SPYTypeError), (np.array([[1, 0, np.nan]]), SPYTypeError),
    (np.array([["a", "b", "c"]]), SPYTypeError), (np.zeros((3, 2), dtype=int), SPYValueError),
    (np.zeros((0, 3), dtype=int), SPYValueError), (np.zeros(3, dtype=int), SPYValueError),
])
def test_spikedata_refuses(bad, exc):
    with pytest.raises(exc):
        spy.SpikeData(bad, samplerate=1.0)


def test_spikedata_other_errors_and_samples_above_2_31():
    with pytest.raises(SPYValueError):
        spy.SpikeData([[1, 0, 0]], samplerate=1.0, dimord=["sample", "channel", "neuron"])
    d = spy.SpikeData([[3_000_000_000, 0, 0]], samplerate=1.0, trialdefinition=[[2_999_999_999, 3_000_000_001, 0]])
    assert d.trial_rows.tolist() == [[0, 1]]
    d.data = [[5, 0, 0], [4, 1, 1]]                               # assigning sorts again and finds the trials again
    assert d.data.tolist() == [[4, 1, 1], [5, 0, 0]] and d.trial_rows.tolist() == [[2, 2]]


def test_poisson_noise_is_the_reference_generator():
    a = spy.synthdata.poisson_noise(nTrials=5, nSpikes=2000, seed=42)
    b = spy.synthdata.poisson_noise(nTrials=5, nSpikes=2000, seed=42)
    assert isinstance(a, spy.SpikeData) and np.array_equal(a.data, b.data)
    assert np.array_equal(a.trialdefinition, b.trialdefinition)
    assert not np.array_equal(a.data, spy.synthdata.poisson_noise(nTrials=5, nSpikes=2000, seed=43).data)
    # the draws of syncopy/synthdata/spikes.py, in its order
    rng = np.random.default_rng(42)
    samples = np.sort(rng.choice(range(20000), size=2000, replace=False))
    w = np.random.default_rng(42).uniform(size=3)
    chans = rng.choice(np.arange(3), p=w / w.sum(), size=2000, replace=True)
    w = np.random.default_rng(42).uniform(size=10)
    units = rng.choice(np.arange(10), p=w / w.sum(), size=2000, replace=True)
    assert np.array_equal(a.data, np.stack([samples, chans, units], axis=1))
    end = np.arange(4000, 20001, 4000) - 1 - np.r_[rng.integers(400, size=4), 0]
    assert np.array_equal(a.trialdefinition[:, 1], end) and np.array_equal(a.trialdefinition[:, 0], np.arange(5) * 4000)
    assert a.samplerate == 10000 and np.all(a.trialdefinition[:, 2] < 0)


def test_container_still_refuses_spike_data(tmp_path):
    with pytest.raises((SPYError, TypeError)):
        spy.save(_data(), filename=str(tmp_path / "x.spike"))
    with pytest.raises(SPYError):
        spy.load(str(tmp_path / "x.spike"))
