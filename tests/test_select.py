"""spy.selectdata, spy.copy and spy.redefinetrial (syncopy_amd/datatype/selectdata.py, redefinetrial.py, csrc/select.hip)
without a GPU: the front end's planner against the NumPy model of tests/select_oracle.py for the four data classes, the
route table through its shim, every error path, the latency trial discard, the bookkeeping of redefinetrial, and the
library's own launcher and kernels at their dispatch edges through the CPU emulation (tests/emu/select_emu.cpp)."""
import numpy as np
import pytest

import select_drive as SD
import select_oracle as SO
import syncopy_amd as spy
from syncopy_amd.datatype import Selection, selectdata as S
from syncopy_amd.shared import latency as L
from syncopy_amd.shared.errors import SPYError, SPYTypeError, SPYValueError


@pytest.fixture(scope="module")
def emu():
    return SD.emu()


@pytest.fixture
def on_emulator(emu, monkeypatch):
    """spy.selectdata computed by the emulated library with two workgroups per launch"""
    monkeypatch.setattr(S, "_run", SD.emu_run(emu.few))


@pytest.fixture(scope="module")
def gather(emu):
    return SD.emu_gather(emu.few)


# ---- the front end against the oracle ----------------------------------------------------------------------------------------
def test_front_ends_exist(on_emulator):
    """none of the three existed before"""
    x = SD.make("AnalogData")
    res = spy.selectdata(x, trials=[1])
    SD.same_bits(res.data, x.data[10:22])
    assert callable(spy.copy) and callable(spy.redefinetrial)


@pytest.mark.parametrize("case", range(len(SD.FRONT_CASES)), ids=[c[0] + str(i) for i, c in enumerate(SD.FRONT_CASES)])
def test_plan_against_oracle(case, on_emulator):
    cls, kwargs = SD.FRONT_CASES[case]
    obj = SD.make(cls)
    keep = obj.data.copy()
    SD.check_frontend(obj, obj, kwargs)
    SD.same_bits(obj.data, keep)


@pytest.mark.parametrize("name", list(SD.DT))
def test_dtypes(name, on_emulator):
    for cls in ("AnalogData", "SpectralData"):
        obj = SD.make(cls, SD.DT[name])
        res = SD.check_frontend(obj, obj, {"trials": [2, 0], "channel": [4, 1]})
        assert res.data.dtype == SD.DT[name]


def test_plan_tables():
    """what the planner hands to the kernel: rows of the selected windows, one spec per inner axis"""
    s = SD.make("SpectralData")
    p = S._plan(s, trials=[2, 0], latency=[-0.1, 0.1], taper=[3, 0], frequency=[30, 60], channel=slice(1, 3))
    assert p.rows == [(10, 13), (1, 4)] and list(p.starts) == [0, 3] and p.nrows == 6
    assert p.inner == (2, 4, 2) and p.full == (4, 9, 5)
    assert list(p.axes[0]) == [3, 0] and p.axes[1] == (3, 4) and p.axes[2] == (1, 2)
    assert np.array_equal(p.trialdefinition, [[0, 3, -1], [3, 6, -1]])
    p = S._plan(s, channel=[0, 1, 2, 3, 4], frequency=40)
    assert p.axes == [None, (4, 1), None]                                    # a list that is the whole axis is no list
    a = SD.make("AnalogData")
    assert S._plan(a).axes == [None] and S._plan(a).rows == [(1, 10), (10, 22), (23, 30), (30, 41)]


def test_existing_selection_is_left_alone(on_emulator):
    x = SD.make("AnalogData")
    x.selectdata({"trials": [3, 0], "channel": [1]})
    mine = x.selection
    res = SD.check_frontend(x, x, {"trials": [1], "latency": [-0.2, 0.2]})
    assert x.selection is mine and res.data.shape == (5, 6)                  # the keywords alone decide, as in the reference


def test_latency_discards_trials(on_emulator):
    """trials cover [-0.3, 0.5], [-0.4, 0.7], [-0.3, 0.3] and [-0.5, 0.5] seconds"""
    x = SD.make("AnalogData")
    assert L.get_analysis_window(x, "minperiod") == [-0.3, 0.3] and L.get_analysis_window(x, "maxperiod") == [-0.5, 0.7]
    assert L.get_analysis_window(x, "prestim") == [-0.5, 0] and L.get_analysis_window(x, "poststim") == [0, 0.7]
    sel, gone = L.create_trial_selection(x, [-0.3, 0.5])
    assert list(sel["trials"]) == [0, 1, 3] and gone == 1
    x.selectdata({"trials": [3, 2, 1, 3], "channel": [0]})                   # an in-place selection is respected
    assert L.get_analysis_window(x, "minperiod") == [-0.3, 0.3]
    sel, gone = L.create_trial_selection(x, [-0.4, 0.5])
    assert list(sel["trials"]) == [3, 1, 3] and gone == 1 and sel["channel"] == [0]
    x.selection = None
    res = spy.selectdata(x, latency=[-0.35, 0.45])
    assert np.array_equal(res.trialdefinition, [[0, 8, -3, 8], [8, 16, -3, 10]])
    SD.same_bits(res.data, np.concatenate([x.data[11:19], x.data[32:40]]))
    res = spy.selectdata(x, trials=[2, 1], latency="maxperiod")                # [-0.4, 0.7]: trial 2 goes
    assert np.array_equal(res.trialdefinition, [[0, 12, -4, 8]])
    res = spy.selectdata(x, latency=[0.0, 0.0])                               # a window that keeps one row per trial
    assert np.array_equal(res.trialdefinition[:, :3], [[0, 1, 0], [1, 2, 0], [2, 3, 0], [3, 4, 0]])
    SD.same_bits(res.data, x.data[[4, 14, 26, 35]])
    assert np.array_equal(spy.selectdata(x, latency="all").trialdefinition[:, 1], [9, 21, 28, 39])
    with pytest.raises(SPYValueError, match="expected at least one trial covering the latency window"):
        spy.selectdata(x, latency=[-0.5, 0.7])
    with pytest.raises(SPYValueError, match="start of latency window"):
        spy.selectdata(x, latency=[2.0, 3.0])
    with pytest.raises(SPYValueError, match="end of latency window"):
        spy.selectdata(x, latency=[-3.0, -2.0])
    with pytest.raises(SPYValueError, match="start < end latency window"):
        spy.selectdata(x, latency=[0.2, -0.2])
    with pytest.raises(SPYValueError, match="of `latency`"):
        spy.selectdata(x, latency="sometime")
    with pytest.raises(SPYValueError, match="of `latency`"):
        spy.selectdata(x, latency=[0.0, 0.1, 0.2])


# ---- error paths ---------------------------------------------------------------------------------------------------------------
def test_keys_per_class():
    a, s, c, t = (SD.make(k) for k in ("AnalogData", "SpectralData", "CrossSpectralData", "TimeLockData"))
    for obj, bad in ((a, {"frequency": 10}), (a, {"taper": 0}), (a, {"channel_i": 0}), (t, {"frequency": [10, 20]}),
                     (t, {"channel_j": 0}), (s, {"channel_i": [0]}), (s, {"channel_j": [0]}), (c, {"channel": [0]}),
                     (c, {"taper": [0]})):
        key = list(bad)[0]
        with pytest.raises(SPYValueError, match=f"no `{key}` selection available for {type(obj).__name__}"):
            spy.selectdata(obj, **bad)
    with pytest.raises(SPYValueError, match="selection kwargs.*trails"):
        spy.selectdata(a, trails=[0])
    with pytest.raises(SPYValueError, match="`select` as explicit parameter"):
        spy.selectdata(a, select={"trials": [0]})
    spikes = spy.SpikeData(np.array([[1, 0, 0], [3, 1, 0]]), samplerate=10.0, trialdefinition=[[0, 5, 0]])
    for f in (spy.selectdata, spy.copy, spy.redefinetrial):
        with pytest.raises(SPYTypeError, match="of `data`"):
            f(spikes)
        with pytest.raises(SPYTypeError, match="of `data`"):
            f(np.ones((3, 2)))
    with pytest.raises(SPYTypeError, match="of `inplace`"):
        spy.selectdata(a, inplace=1)
    with pytest.raises(SPYTypeError, match="of `clear`"):
        spy.selectdata(a, clear="yes")
    with pytest.raises(SPYValueError, match="non-empty Syncopy data object"):
        spy.selectdata(spy.AnalogData())
    with pytest.raises(SPYTypeError, match="float32, float64, complex64 or complex128 data"):
        spy.selectdata(spy.AnalogData(np.ones((4, 2), dtype=np.int16), samplerate=1.0))


def test_selector_errors():
    a, s, c = SD.make("AnalogData"), SD.make("SpectralData"), SD.make("CrossSpectralData")
    with pytest.raises(SPYValueError, match="trial indices in"):
        spy.selectdata(a, trials=[4])
    with pytest.raises(SPYValueError, match="existing channel names"):
        spy.selectdata(a, channel=["ch1", "nope"])
    with pytest.raises(SPYValueError, match=r"channel indices in \[0, 6\)"):
        spy.selectdata(a, channel=[0, 6])
    with pytest.raises(SPYValueError, match="channel indices or names"):
        spy.selectdata(a, channel=[0.5])
    with pytest.raises(SPYValueError, match="at least one selected channel"):
        spy.selectdata(a, channel=slice(4, 2))
    with pytest.raises(SPYValueError, match="existing taper names"):
        spy.selectdata(s, taper="t9")
    with pytest.raises(SPYValueError, match=r"taper indices in \[0, 4\)"):
        spy.selectdata(s, taper=[-1])
    with pytest.raises(SPYValueError, match=r"channel_i indices in \[0, 4\)"):
        spy.selectdata(c, channel_i=range(3, 6))
    with pytest.raises(SPYValueError, match="existing channel_j names"):
        spy.selectdata(c, channel_j=["a0"])
    for bad in (-1.0, 81, [30, 90], [-5, 20], [1, 2, 3], [np.nan, 20], np.inf, "low", [[10, 20]]):
        with pytest.raises(SPYValueError, match="of `frequency`"):
            spy.selectdata(s, frequency=bad)
    for bad in ([40, 40], [60, 30]):
        with pytest.raises(SPYValueError, match=r"`frequency\[0\]` < `frequency\[1\]`"):
            spy.selectdata(c, frequency=bad)
    with pytest.raises(SPYValueError, match="at least one selected frequency"):
        spy.selectdata(s, frequency=[31, 39])
    assert S._plan(s, frequency="all").axes[1] is None and S._plan(s, frequency=44.9).axes[1] == (4, 1)
    assert S._plan(s, frequency=45.0).axes[1] == (5, 1)                       # a tie goes to the right neighbour
    s.freq = None
    with pytest.raises(SPYValueError, match="Syncopy data object with freq-dimension"):
        spy.selectdata(s, frequency=10)


def test_inplace_and_clear():
    x = SD.make("AnalogData")
    assert spy.selectdata(x, trials=[3, 2, 0], channel=["ch2", "ch0"], latency=[-0.3, 0.5], inplace=True) is None
    assert isinstance(x.selection, Selection) and x.selection.trial_ids == [3, 0] and x.selection.channel == [2, 0]
    assert x.selection.time == {3: (2, 11), 0: (0, 9)}                        # trial 2 did not cover the window
    assert x.cfg["selectdata"]["inplace"] is True
    assert spy.selectdata(x, clear=True) is None and x.selection is None
    assert spy.selectdata(x, clear=True) is None
    with pytest.raises(SPYValueError, match="no data selectors if `clear = True`"):
        spy.selectdata(x, trials=[0], clear=True)
    s, c = SD.make("SpectralData"), SD.make("CrossSpectralData")
    for obj, bad in ((s, {"frequency": [10, 20]}), (s, {"taper": [0]}), (s, {"trials": [0], "taper": [0]}),
                     (c, {"channel_i": [0]}), (c, {"channel_j": [0]}), (c, {"frequency": 10})):
        with pytest.raises(SPYValueError, match="a deep copy is needed"):
            spy.selectdata(obj, inplace=True, **bad)
        assert obj.selection is None
    spy.selectdata(s, trials=[2, 0], channel=[1], inplace=True)
    assert s.selection.trial_ids == [2, 0] and s.selection.channel == [1]
    spy.selectdata(c, trials=[1], inplace=True)
    assert c.selection.trial_ids == [1]
    # the existing method of the classes is what it was
    y = SD.make("AnalogData").selectdata({"trials": [1], "latency": [-0.5, 0.9]})
    assert y.selection.trial_ids == [1] and y.selection.time == {1: (0, 12)}


# ---- copy and redefinetrial ---------------------------------------------------------------------------------------------------
def test_copy_on_the_host():
    for cls in ("AnalogData", "SpectralData", "CrossSpectralData", "TimeLockData"):
        x = SD.make(cls)
        x.cfg = {"a": 1}
        if cls == "TimeLockData":
            x.avg = np.ones((3, 6), dtype=np.float32)
        y = spy.copy(x)
        assert type(y) is type(x) and y is not x and y.data is not x.data and y.cfg == {"a": 1} and y.cfg is not x.cfg
        SD.same_bits(y.data, x.data)
        assert np.array_equal(y.trialdefinition, x.trialdefinition) and y.trialdefinition is not x.trialdefinition
        for prop in ("channel", "freq", "taper", "channel_i", "channel_j", "avg"):
            if getattr(x, prop, None) is not None:
                assert list(np.ravel(getattr(y, prop))) == list(np.ravel(getattr(x, prop))) and getattr(y, prop) is not getattr(x, prop)
        y.data[0] = 0
        assert not np.array_equal(y.data[0], x.data[0])
    assert spy.copy(spy.AnalogData()).data is None


def test_redefinetrial_bookkeeping(on_emulator):
    """hand-computed trialdefinitions; the source's trials are rows [1, 10), [10, 22), [23, 30), [30, 41) with offsets
    -3, -4, -3, -5 and a fourth column 7 ... 10"""
    x = SD.make("AnalogData")
    x.cfg = {"earlier": True}
    keep, trl0 = x.data.copy(), x.trialdefinition.copy()
    r = spy.redefinetrial(x)                                                  # a copy and nothing else
    assert np.array_equal(r.trialdefinition, trl0) and r.data is not x.data and r.cfg["earlier"] is True
    assert r.cfg["redefinetrial"] == {"trials": None, "minlength": None, "offset": None, "toilim": None, "begsample": None,
                                      "endsample": None, "trl": None}
    r = spy.redefinetrial(x, trials=[3, 0])
    assert np.array_equal(r.trialdefinition, [[0, 11, -5, 10], [11, 20, -3, 7]])
    SD.same_bits(r.data, np.concatenate([x.data[30:41], x.data[1:10]]))
    r = spy.redefinetrial(x, toilim=[-0.2, 0.3])                              # all four trials cover it
    assert np.array_equal(r.trialdefinition, [[0, 6, -2, 7], [6, 12, -2, 8], [12, 18, -2, 9], [18, 24, -2, 10]])
    SD.same_bits(r.data, np.concatenate([x.data[2:8], x.data[12:18], x.data[24:30], x.data[33:39]]))
    r = spy.redefinetrial(x, trials=[1, 2], toilim=[-0.4, 0.4])               # trial 2 does not
    assert np.array_equal(r.trialdefinition, [[0, 9, -4, 8]])
    r = spy.redefinetrial(x, minlength=1.0)                                   # 10 samples: trials 1 and 3
    assert np.array_equal(r.trialdefinition, [[0, 12, -4, 8], [12, 23, -5, 10]])
    assert spy.redefinetrial(x, minlength=5.0).data is None                   # an empty object
    r = spy.redefinetrial(x, begsample=2, endsample=5)
    assert np.array_equal(r.trialdefinition, [[3, 6, -3, 7], [12, 15, -4, 8], [25, 28, -3, 9], [32, 35, -5, 10]])
    SD.same_bits(r.data, x.data)
    r = spy.redefinetrial(x, trials=[2, 0], begsample=[0, 3], endsample=[7, 3], offset=np.array([-1, 0]))
    assert np.array_equal(r.trialdefinition, [[0, 7, -1, 9], [10, 10, 0, 7]])   # the second trial has no rows
    r = spy.redefinetrial(x, offset=-2)
    assert np.array_equal(r.trialdefinition[:, 2], [-2] * 4) and np.array_equal(r.trialdefinition[:, :2], trl0[:, :2])
    r = spy.redefinetrial(x, trl=[0, 43, -7])
    assert np.array_equal(r.trialdefinition, [[0, 43, -7]])
    r = spy.redefinetrial(x, trials=[1], trl=[[0, 5, 0], [5, 12, -1]])
    assert np.array_equal(r.trialdefinition, [[0, 5, 0], [5, 12, -1]]) and r.data.shape == (12, 6)
    s = spy.redefinetrial(SD.make("SpectralData"), trials=[2], begsample=1, endsample=4)
    assert isinstance(s, spy.SpectralData) and np.array_equal(s.trialdefinition, [[1, 4, -2]])
    SD.same_bits(x.data, keep)
    assert np.array_equal(x.trialdefinition, trl0) and x.selection is None and x.cfg == {"earlier": True}


def test_redefinetrial_errors(on_emulator):
    x = SD.make("AnalogData")
    for bad in ({"minlength": 1, "toilim": [0, 1]}, {"toilim": [0, 1], "begsample": 0, "endsample": 2},
                {"trl": [0, 5, 0], "minlength": 1}, {"begsample": 0, "endsample": 1, "trl": [0, 5, 0]}):
        with pytest.raises(SPYError, match="Incompatible input arguments, either `minlength`"):
            spy.redefinetrial(x, **bad)
    with pytest.raises(SPYError, match="either complete trialdefinition `trl`"):
        spy.redefinetrial(x, trl=[0, 5, 0], offset=1)
    with pytest.raises(SPYValueError, match="both `begsample` and `endsample`"):
        spy.redefinetrial(x, begsample=1)
    with pytest.raises(SPYValueError, match="relative `begsample` < 0"):
        spy.redefinetrial(x, begsample=-1, endsample=2)
    with pytest.raises(SPYValueError, match="wrong sized `begsample`"):
        spy.redefinetrial(x, begsample=[0, 1], endsample=[2, 3])
    with pytest.raises(SPYValueError, match="different sizes"):
        spy.redefinetrial(x, begsample=0, endsample=[1, 2, 3, 4])
    with pytest.raises(SPYValueError, match="of `endsample`: 'out of range'"):
        spy.redefinetrial(x, begsample=0, endsample=14)                       # 30 + 14 > 43
    with pytest.raises(SPYValueError, match="endsample < begsample"):
        spy.redefinetrial(x, begsample=3, endsample=2)
    with pytest.raises(SPYTypeError, match="of `begsample`"):
        spy.redefinetrial(x, begsample="a", endsample=2)
    with pytest.raises(SPYValueError, match="array of length 4"):
        spy.redefinetrial(x, offset=np.array([0, 1]))
    with pytest.raises(SPYTypeError, match="of `offset`"):
        spy.redefinetrial(x, offset=[0, 1, 2, 3])
    with pytest.raises(SPYValueError, match="of `trials`"):
        spy.redefinetrial(x, trials=[0.5])
    with pytest.raises(SPYValueError, match="of `toilim`"):
        spy.redefinetrial(x, toilim=[0, 1, 2])
    with pytest.raises(SPYValueError, match="of `minlength`"):
        spy.redefinetrial(x, minlength=-1)
    with pytest.raises(SPYValueError, match="of `minlength`"):
        spy.redefinetrial(x, minlength="maxperlen")
    for bad in ([0, 44, 0], [-1, 5, 0], [0.5, 5, 0], [[0, 5]], [5, 2, 0]):
        with pytest.raises(SPYValueError, match="of `trl`"):
            spy.redefinetrial(x, trl=bad)
    with pytest.raises(SPYValueError, match="non-empty Syncopy data object"):
        spy.redefinetrial(spy.AnalogData())


def test_a_trial_without_rows_can_be_selected(on_emulator):
    x = spy.redefinetrial(SD.make("AnalogData"), begsample=[0, 4, 0, 0], endsample=[3, 4, 2, 5])
    res = SD.check_frontend(x, x, {"trials": [0, 1, 2], "channel": [5, 0]})
    assert np.array_equal(res.trialdefinition[:, :3], [[0, 3, -3], [3, 3, 0], [3, 5, -3]])


# ---- the route ---------------------------------------------------------------------------------------------------------------
def test_route_collapse():
    """adjacent whole axes merge, a whole axis merges into a range to its left, axes of extent 1 drop out"""
    tr = [(0, 4)]
    r = SD.route(4, 4, (3, 5, 8), tr, None)
    assert (r.mode, r.run, r.wo, r.ws) == (SD.FLAT, 120, 120, 120)
    r = SD.route(4, 4, (3, 5, 8), tr, [(0, 3), None, (0, 8)])                 # ranges that cover their axes are whole
    assert (r.mode, r.run) == (SD.FLAT, 120)
    r = SD.route(4, 4, (3, 5, 8), tr, [(1, 2), None, None])
    assert (r.mode, r.run, r.n, r.s, r.start, r.wo) == (SD.AXES, 80, [1, 1, 80], [0, 0, 1], [0, 0, 40], 80)
    r = SD.route(4, 4, (3, 5, 8), tr, [None, (1, 2), None])
    assert (r.run, r.n, r.s, r.start) == (16, [1, 3, 16], [0, 40, 1], [0, 0, 8])
    r = SD.route(4, 4, (3, 5, 8), tr, [None, None, (2, 3)])
    assert (r.run, r.n, r.s, r.start) == (3, [1, 15, 3], [0, 8, 1], [0, 0, 2])
    r = SD.route(4, 4, (3, 5, 8), tr, [[2, 0], None, None])
    assert (r.mode, r.run, r.n, r.s, r.loff, r.nidx) == (SD.AXES_LDS, 40, [1, 2, 40], [0, 40, 1], [-1, 0, -1], 2)
    r = SD.route(4, 4, (3, 5, 8), tr, [[2, 0], (1, 2), [7, 7, 1]])
    assert (r.run, r.n, r.s, r.start, r.loff, r.nidx) == (1, [2, 2, 3], [40, 8, 1], [0, 1, 0], [0, -1, 2], 5)
    r = SD.route(8, 4, (1, 6, 1), tr, [None, [5, 0], None])
    assert (r.run, r.n, r.loff) == (1, [1, 1, 2], [-1, -1, 0])
    r = SD.route(4, 4, (1, 5), tr, [[0, 0, 0], None])                          # a list that repeats the one entry stays
    assert (r.mode, r.run, r.wo, r.ws, r.n, r.s, r.loff, r.nidx) == (SD.AXES_LDS, 5, 15, 5, [1, 3, 5], [0, 5, 1], [-1, 0, -1], 3)
    r = SD.route(4, 4, (1, 5), tr, [[0], None])                                # one entry of one: the axis drops out
    assert (r.mode, r.run, r.wo, r.ws) == (SD.FLAT, 5, 5, 5)
    r = SD.route(4, 4, (1, 1, 1), tr, [[0, 0], None, [0, 0, 0]])
    assert (r.mode, r.wo, r.ws, r.n, r.s, r.loff) == (SD.AXES_LDS, 6, 1, [1, 2, 3], [0, 1, 1], [-1, 0, 2])
    r = SD.route(4, 4, (6,), tr, [(2, 3)])
    assert (r.mode, r.run, r.n, r.start, r.ws) == (SD.AXES, 3, [1, 1, 3], [0, 0, 2], 6)
    cap = SD.lds_cap()
    assert cap == 4096
    assert SD.route(4, 4, (3, 2), tr, [np.zeros(cap, dtype=np.int32), None]).mode == SD.AXES_LDS
    assert SD.route(4, 4, (3, 2), tr, [np.zeros(cap - 1, dtype=np.int32), [1]]).mode == SD.AXES_LDS
    assert SD.route(4, 4, (3, 2), tr, [np.zeros(cap, dtype=np.int32), [1]]).mode == SD.AXES


def test_route_lanes():
    """16-byte lanes need the run's length and every run's byte offset in both tensors to be multiples of 16"""
    tr = [(0, 4)]
    assert SD.route(4, 4, (8,), tr, None).lane == 16 and SD.route(4, 4, (8,), tr, None, src_addr=4).lane == 4
    assert SD.route(4, 4, (8,), tr, None, out_addr=(1 << 20) + 8).lane == 4
    assert SD.route(8, 4, (8,), tr, None, src_addr=8).lane == 8
    r = SD.route(16, 4, (8,), tr, None, src_addr=8)
    assert r.lane == 16 and not r.aligned and SD.route(16, 4, (8,), tr, None).aligned
    assert SD.route(4, 4, (8,), tr, [(4, 4)]).lane == 16 and SD.route(4, 4, (8,), tr, [(2, 4)]).lane == 4
    assert SD.route(4, 4, (8,), tr, [(0, 6)]).lane == 4 and SD.route(8, 4, (8,), tr, [(0, 6)]).lane == 16
    assert SD.route(4, 4, (7,), tr, [(0, 4)]).lane == 4 and SD.route(4, 9, (7,), [(4, 5)], [(0, 4)]).lane == 16
    assert SD.route(4, 9, (7,), [(4, 5), (8, 9)], [(0, 4)]).lane == 16        # rows 4 and 8 both start on the boundary
    assert SD.route(4, 9, (7,), [(4, 5), (6, 7)], [(0, 4)]).lane == 4
    assert SD.route(4, 9, (7,), [(3, 4)], [(3, 4)]).lane == 16                # element 21 + 3 = 24
    assert SD.route(4, 4, (5, 4), tr, [[4, 1, 1], None]).lane == 16
    assert SD.route(4, 4, (5, 4), tr, [None, [0, 1, 3, 2]]).lane == 4         # a list on the fastest axis: element lanes
    assert SD.route(4, 4, (5, 6), tr, [[4, 2], (0, 4)]).lane == 4             # rows of 30 elements: every second one is off
    assert SD.route(4, 1, (5, 6), [(0, 1)], [[4, 2], (0, 4)]).lane == 16      # 24 and 12
    assert SD.route(4, 1, (5, 6), [(0, 1)], [[4, 1], (0, 4)]).lane == 4       # 24 and 6
    assert SD.route(4, 1, (5, 6), [(0, 1)], [[1, 3], (2, 4)]).lane == 16      # 6 + 2 and 18 + 2
    # whole trials: the trial is the run
    assert SD.route(4, 8, (7,), [(0, 4), (4, 8)], None).lane == 16 and SD.route(4, 8, (7,), [(0, 3), (4, 8)], None).lane == 4
    assert SD.route(4, 8, (7,), [(1, 5)], None).lane == 4 and SD.route(4, 8, (7,), [(4, 8), (2, 2), (0, 4)], None).lane == 16


def test_route_refuses():
    """what the launcher answers with -1 before anything runs"""
    tr = [(0, 4)]
    ok = dict(elem_bytes=4, src_rows=4, inner=(3, 5), trials=tr, axes=None)
    assert SD.route(**ok) is not None
    for eb in (1, 2, 3, 12, 32, 0):
        assert SD.route(**{**ok, "elem_bytes": eb}) is None
    assert SD.route(**ok, src_addr=1 << 20, out_addr=1 << 20) is None         # the output is the source
    for src_addr, out_addr in ((1 << 20, (1 << 20) + 236), ((1 << 20) + 236, 1 << 20), (1 << 20, (1 << 20) - 236)):
        assert SD.route(**ok, src_addr=src_addr, out_addr=out_addr) is None   # 240 bytes each: they overlap by 4
    assert SD.route(**ok, src_addr=1 << 20, out_addr=(1 << 20) + 240) is not None
    assert SD.route(**ok, src_addr=(1 << 20) + 240, out_addr=1 << 20) is not None
    assert SD.route(**ok, src_addr=2) is None and SD.route(**{**ok, "elem_bytes": 8}, out_addr=(1 << 20) + 4) is None
    assert SD.route(**{**ok, "trials": [(0, 5)]}) is None and SD.route(**ok, out_rows=3) is None
    assert SD.route(**ok, desc=[[0, -1, 2]]) is None and SD.route(**ok, desc=[[0, 0, -1]]) is None
    assert SD.route(**ok, desc=[[0, 0, 2], [3, 0, 1]], out_rows=4) is None    # output rows not stacked
    assert SD.route(**ok, desc=[[0, 0, 2], [1, 0, 1]], out_rows=4) is None
    assert SD.route(**ok, desc=[[1, 0, 2], [3, 0, 1]], out_rows=4) is not None
    for axes in ([(0, 4), None], [(3, 1), None], [(-1, 2), None], [None, (4, 2)], [None, [5]], [[-1], None], [[0, 3], None]):
        assert SD.route(**{**ok, "axes": axes}) is None, axes
    assert SD.route(**{**ok, "axes": [(1, 0), None]}) is None                 # a count of 0
    assert SD.route(**{**ok, "axes": [np.zeros(0, dtype=np.int32), None]}) is None
    assert SD.route(**{**ok, "inner": (0, 5)}) is None


def test_launcher_refuses(emu):
    src, out = SD.values((4, 3, 5), np.float32), np.zeros((4, 3, 5), dtype=np.float32)
    desc = SD.table([(0, 4)])
    assert SD.emu_select(src, desc, out) == 0
    SD.same_bits(out, src)
    assert SD.emu_select(src, desc, src) == -1
    both = np.zeros((6, 3, 5), dtype=np.float32)
    assert SD.emu_select(both[:4], desc, both[2:]) == -1                       # the output begins inside the source
    assert SD.emu_select(both[:3], SD.table([(0, 3)]), both[3:]) == 0
    assert SD.emu_select(src, SD.table([(0, 5)]), out) == -1
    assert SD.emu_select(src, desc, out[:3]) == -1
    assert SD.emu_select(src, [[0, 0, 2], [3, 0, 1]], out) == -1
    assert SD.emu_select(src, desc, np.zeros((4, 1, 5), dtype=np.float32), [[3], None]) == -1
    assert SD.emu_select(src, desc, np.zeros((4, 2, 5), dtype=np.float32), [(2, 2), None]) == -1
    assert SD.emu_select(src.view(np.uint16).reshape(4, 3, 10), desc, out.view(np.uint16).reshape(4, 3, 10)) == -1
    assert SD.emu_select(src, np.zeros((0, 3), dtype=np.int64), out) == 0     # no trials: nothing to do


# ---- the kernels at their dispatch edges, emulated ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SD.DT))
def test_element_sizes(gather, name):
    SD.check_element_sizes(gather, name)


def test_sixteen_byte_boundary(gather):
    SD.check_boundary(gather)


def test_trials(gather):
    SD.check_trials(gather)


def test_index_lists(gather):
    SD.check_index_lists(gather)


def test_workgroups_walk_several_rounds(emu):
    """two workgroups over 3 x 257 x 3 elements: each walks two rounds and the last one is short; and the launch log"""
    import build_emu
    src = SD.values((5, 257, 3), np.float32, 8)
    build_emu.launches(emu)
    got, _, _ = SD.emu_gather(emu.few)(src, [(1, 3), (4, 5)], [None, [2, 0, 1]])
    SD.same_bits(got, SO.gather(src, [(1, 3), (4, 5)], [None, [2, 0, 1]]))
    log = build_emu.launches(emu)
    assert log.shape[0] == 1 and list(log[0, :4]) == [2, 1, 1, 256]
    got, _, _ = SD.emu_gather(emu.ctx)(src, [(0, 4)], None)                   # 771 lanes of 16 bytes
    SD.same_bits(got, src[:4])
    assert list(build_emu.launches(emu)[0, :4]) == [4, 1, 1, 256]
