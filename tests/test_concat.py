"""spy.concat (syncopy_amd/datatype/concat.py, csrc/concat.hip) without a GPU: the library's own launcher and kernel at
their dispatch edges through the CPU emulation (tests/emu/concat_emu.cpp), the route through its shim with every refusal
and its text, and the front end's checks and plan against the NumPy model of tests/concat_oracle.py.  Every comparison is
bit for bit."""
import numpy as np
import pytest

import concat_drive as CD
import concat_oracle as CO
import syncopy_amd as spy
from syncopy_amd.datatype import concat as K
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError


@pytest.fixture(scope="module")
def emu():
    return CD.emu()


@pytest.fixture
def on_emulator(emu, monkeypatch):
    """spy.concat computed by the emulated library with two workgroups per launch"""
    monkeypatch.setattr(K, "_run", CD.emu_run(emu.few))


@pytest.fixture(scope="module")
def join(emu):
    return CD.emu_join(emu.ctx)


# ---- the kernel through the library's launcher -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CD.DT))
def test_element_sizes(name, join):
    CD.check_element_sizes(join, name)


def test_lane_width(join):
    CD.check_lanes(join)


def test_layouts(join):
    CD.check_layouts(join)


def test_number_of_sources(join):
    CD.check_sources(join)


def test_trial_tables(join):
    CD.check_trials(join)


def test_two_workgroups(emu):
    """two workgroups of 256 threads on outputs of about 1536 lanes: each walks three rounds"""
    import build_emu
    CD.check_few_workgroups(CD.emu_join(emu.few))
    src = CD._sources((2, 3), (), (701, 835), np.float32, 1)           # 1536 element lanes
    build_emu.launches(emu)
    CD.emu_join(emu.few)(src, [[(1, 2)], [(2, 3)]], 1)
    assert build_emu.launches(emu)[:, :4].tolist() == [[2, 1, 1, CD.THREADS]]   # one launch, capped
    CD.emu_join(emu.ctx)(src, [[(1, 2)], [(2, 3)]], 1)
    assert build_emu.launches(emu)[:, :4].tolist() == [[6, 1, 1, CD.THREADS]]


def test_one_launch_whatever_the_trials_and_sources(emu):
    import build_emu
    src = CD._sources(tuple(range(20, 28)), (2,), (1, 2, 3, 4, 5, 6, 7, 8), np.float32, 2)
    trials = [[(k, k + 2) for k in range(0, 18, 2)] for _ in src]
    build_emu.launches(emu)
    CD.check_case(CD.emu_join(emu.ctx), src, trials, 2, 4)
    assert build_emu.launches(emu).shape[0] == 1


def test_only_the_launch_rows_are_written(emu):
    """a launch whose trials begin at output row 3 (a chunk of the front end) leaves the other rows alone"""
    a, b = CD._sources((5, 5), (), (4, 8), np.float32, 1)
    out = np.full((9, 12), 7.0, dtype=np.float32)
    desc = CD.table([[(0, 2), (2, 5)], [(3, 5), (0, 3)]], first=3)
    assert CD.emu_concat([a, b], desc, out) == 0
    CD.same_bits(out[3:8], CO.join([a, b], [[(0, 2), (2, 5)], [(3, 5), (0, 3)]], 1))
    assert np.all(out[:3] == 7.0) and np.all(out[8:] == 7.0)


# ---- the route -----------------------------------------------------------------------------------------------------------------
OK = dict(elem_bytes=4, src_rows=[4, 6], run=[3, 5], pre=2, desc=[[0, 4, 0, 2]])


def test_route_tables():
    r = CD.route(**OK)
    assert r.err is None and (r.lane, r.w, r.row0, r.nrows, r.cum[:3]) == (4, 8, 0, 4, [0, 3, 8])
    r = CD.route(8, [4, 6, 9], [2, 6, 4], 3, [[2, 3, 0, 2, 6], [5, 0, 4, 6, 9], [5, 1, 3, 0, 8]], out_rows=7)
    assert r.err is None and (r.lane, r.aligned, r.w, r.row0, r.nrows, r.cum[:4]) == (16, True, 12, 2, 4, [0, 2, 8, 12])
    assert CD.route(8, [4, 6], [2, 5], 1, [[0, 1, 0, 0]]).lane == 8
    assert CD.route(4, [4, 6], [4, 8], 1, [[0, 1, 0, 0]], out_addr=(1 << 40) + 4).lane == 4
    r = CD.route(16, [4, 6], [1, 1], 1, [[0, 1, 0, 0]], src_addr=[1 << 32, (2 << 32) + 8])
    assert (r.lane, r.aligned) == (16, False)
    assert CD.route(**{**OK, "desc": np.zeros((0, 4))}).nrows == 0                # no trials: nothing to do
    assert CD.shim().cr_max_sources() == 8


def test_route_refuses():
    """what the launcher answers with -1 before anything runs, and why"""
    nine = dict(elem_bytes=4, src_rows=[4] * 9, run=[1] * 9, pre=1, desc=[[0, 4] + [0] * 9])
    assert CD.route(**nine).err == "the number of sources is not 2 to 8"
    assert CD.route(**{**nine, "nsrc": 8}).err is None
    assert CD.route(4, [4], [3], 1, [[0, 4, 0]]).err == "the number of sources is not 2 to 8"
    assert CD.route(**OK, nsrc=0).err == "the number of sources is not 2 to 8"
    for eb in (1, 2, 3, 12, 32, 0):
        assert CD.route(**{**OK, "elem_bytes": eb}).err == "element size is not 4, 8 or 16 bytes"
    assert CD.route(**{**OK, "run": [3, 0]}).err == "a run is below 1" and CD.route(**{**OK, "run": [-1, 5]}).err == "a run is below 1"
    assert CD.route(**{**OK, "pre": 0}).err == "pre is below 1" and CD.route(**{**OK, "pre": -2}).err == "pre is below 1"
    outside = "a trial lies outside its tensor"
    assert CD.route(**{**OK, "desc": [[0, 4, 1, 2]]}).err == outside            # past the first source's rows
    assert CD.route(**{**OK, "desc": [[0, 4, 0, 3]]}).err == outside            # past the second's
    assert CD.route(**{**OK, "desc": [[0, 4, 0, -1]]}).err == outside and CD.route(**{**OK, "desc": [[0, -1, 0, 0]]}, out_rows=4).err == outside
    assert CD.route(**OK, out_rows=3).err == outside and CD.route(**{**OK, "desc": [[-1, 4, 0, 2]]}, out_rows=8).err == outside
    stacked = "the output rows are not stacked"
    assert CD.route(**{**OK, "desc": [[0, 2, 0, 0], [3, 1, 0, 0]]}, out_rows=4).err == stacked
    assert CD.route(**{**OK, "desc": [[0, 2, 0, 0], [1, 1, 0, 0]]}, out_rows=4).err == stacked
    assert CD.route(**{**OK, "desc": [[1, 2, 0, 0], [3, 1, 0, 0]]}, out_rows=4).err is None
    at = 1 << 20                                                                  # sources of 96 and 240 bytes, an output of 256
    assert CD.route(**OK, src_addr=[at, 2 * at], out_addr=at).err == "the output is a source"
    assert CD.route(**OK, src_addr=[at, 2 * at], out_addr=2 * at).err == "the output is a source"
    overlaps = "the output overlaps a source"
    for src_addr, out_addr in (([at, 2 * at], at + 92), ([at, 2 * at], at - 252), ([2 * at, at], at + 236), ([at, 2 * at], 2 * at - 252)):
        assert CD.route(**OK, src_addr=src_addr, out_addr=out_addr).err == overlaps, (src_addr, out_addr)
    for src_addr, out_addr in (([at, 2 * at], at + 96), ([at, 2 * at], at - 256), ([2 * at, at], at + 240)):
        assert CD.route(**OK, src_addr=src_addr, out_addr=out_addr).err is None, (src_addr, out_addr)
    assert CD.route(**OK, src_addr=[at, at]).err is None                         # sources may be one another
    misaligned = "a tensor is not aligned to its element type"
    assert CD.route(**OK, src_addr=[at + 2, 2 * at]).err == misaligned and CD.route(**OK, out_addr=at + 1).err == misaligned
    assert CD.route(**{**OK, "elem_bytes": 8}, src_addr=[at, 2 * at + 4]).err == misaligned
    assert CD.route(**{**OK, "elem_bytes": 16}, src_addr=[at, 2 * at + 4]).err == misaligned
    assert CD.route(**{**OK, "elem_bytes": 16}, src_addr=[at, 2 * at + 8]).err is None
    big = 1 << 57                                                                 # the guard of select_route: 2^58 elements
    assert CD.route(4, [1, 1], [big, big], 1, [[0, 1, 0, 0]]).err == "a row is too wide"
    assert CD.route(4, [1, 1], [big >> 1, 1], 4, [[0, 1, 0, 0]]).err == "a row is too wide"
    assert CD.route(4, [big, 1], [2, 1], 1, [[0, 1, 0, 0]]).err == "the tensor is too large"
    assert CD.route(4, [1, 1], [2, 1], 1, [[0, 1, 0, 0]], out_rows=big).err == "the tensor is too large"
    assert CD.route(**{**OK, "src_rows": [-1, 6]}).err == "negative row or trial count"


def test_launcher_refuses(emu):
    a, b = CD._sources((4, 6), (), (3, 5), np.float32, 1)
    out = np.zeros((4, 8), dtype=np.float32)
    desc = [[0, 4, 0, 2]]
    assert CD.emu_concat([a, b], desc, out) == 0
    CD.same_bits(out, np.concatenate([a, b[2:]], axis=1))
    assert CD.emu_concat([a], [[0, 4, 0]], out, run=[3]) == -1                    # one source
    nine = [a] * 9
    assert CD.emu_concat(nine, [[0, 4] + [0] * 9], np.zeros((4, 27), dtype=np.float32)) == -1
    assert CD.emu_concat([a, b], desc, out, elem_bytes=2) == -1
    assert CD.emu_concat([a, b], desc, out, run=[3, 0]) == -1 and CD.emu_concat([a, b], desc, out, pre=0, run=[3, 5]) == -1
    assert CD.emu_concat([a, b], [[0, 4, 1, 2]], out) == -1 and CD.emu_concat([a, b], [[0, 4, 0, 3]], out) == -1
    assert CD.emu_concat([a, b], desc, out[:3]) == -1
    assert CD.emu_concat([a, b], [[0, 2, 0, 0], [3, 1, 0, 0]], out) == -1         # output rows not stacked
    both = np.zeros(4 * 8 + 4 * 3, dtype=np.float32)
    src, dst = both[:12].reshape(4, 3), both[:32].reshape(4, 8)
    assert CD.emu_concat([src, b], desc, dst) == -1                              # the output is a source
    assert CD.emu_concat([b, src], [[0, 4, 2, 0]], dst, run=[5, 3]) == -1
    assert CD.emu_concat([both[32:].reshape(4, 3), b], desc, both[1:33].reshape(4, 8)) == -1     # overlaps by one element
    assert CD.emu_concat([both[32:].reshape(4, 3), b], desc, dst) == 0
    assert CD.emu_concat([a, b], np.zeros((0, 4), dtype=np.int64), out) == 0      # no trials: nothing to do


# ---- the front end: checks and plan ---------------------------------------------------------------------------------------------
def test_front_end_exists(on_emulator):
    """it did not exist before"""
    a, b = CD.make_pair(0)
    res = spy.concat(a, b)
    want = np.concatenate([np.concatenate([a.data[p:q], b.data[p + 2:q + 2]], axis=1) for p, q in a.sampleinfo])
    CD.same_bits(res.data, want)
    assert spy._LAZY["concat"] == ".datatype.concat"


@pytest.mark.parametrize("case", range(len(CD.FRONT_CASES)), ids=[c[0] + str(i) for i, c in enumerate(CD.FRONT_CASES)])
def test_plan_against_oracle(case, on_emulator):
    objs = CD.make_pair(case)
    keep = [o.data.copy() for o in objs]
    res = CD.check_frontend(objs, objs)
    assert list(res.channel) == [f"a{i}" for i in range(6)] + [f"b{i}" for i in range(4)]
    for o, k in zip(objs, keep):
        CD.same_bits(o.data, k)
    cls, dimord = CD.FRONT_CASES[case]
    third = CD.make(cls, 1, None, 3, "c", 1, dimord)
    CD.check_frontend(objs + [third], objs + [third])
    CD.check_frontend([third] + objs, [third] + objs)


@pytest.mark.parametrize("name", list(CD.DT))
def test_dtypes(name, on_emulator):
    for case in (0, 2):
        objs = CD.make_pair(case, CD.DT[name])
        assert CD.check_frontend(objs, objs).data.dtype == CD.DT[name]


def test_plan_tables():
    """what the planner hands to the kernel"""
    a, b = CD.make_pair(0)
    p = K._plan([a, b])
    assert p.rows == [[(1, 10), (10, 22), (23, 30), (30, 41)], [(3, 12), (12, 24), (25, 32), (32, 43)]]
    assert list(p.n) == [9, 12, 7, 11] and list(p.starts) == [0, 9, 21, 28] and p.nrows == 39
    assert (p.pre, p.run, p.inner, p.full) == (1, [6, 4], (10,), [(6,), (4,)])
    a, b = CD.make_pair(1)
    p = K._plan([a, b])
    assert (p.pre, p.run, p.inner, p.full, p.axis) == (6, [6, 4], (2, 3, 10), [(2, 3, 6), (2, 3, 4)], 3)
    a, b = CD.make_pair(2)
    p = K._plan([a, b, a])
    assert (p.pre, p.run, p.inner, p.axis) == (1, [36, 24, 36], (16, 2, 3), 1)
    assert list(K._chunks(p, [0, 1, 2], 1 << 30)) == [(0, 3)] and list(K._chunks(p, [], 1)) == [(0, 3)]
    row = (36 + 24) * 8                                                           # bytes of a row of the two host sources
    assert list(K._chunks(p, [0, 1], 9 * row)) == [(0, 2), (2, 3)] and list(K._chunks(p, [0, 1], 1)) == [(0, 1), (1, 2), (2, 3)]


def test_trial_definition_and_cfg(on_emulator):
    a, b = CD.make_pair(0)
    a.cfg = {"earlier": True}
    res = spy.concat(a, b)
    # stacked, with the first object's offsets and fourth column
    assert np.array_equal(res.trialdefinition, [[0, 9, -3, 7], [9, 21, -4, 8], [21, 28, -3, 9], [28, 39, -5, 10]])
    assert res.cfg == {"earlier": True, "concat": {"dim": "channel", "objects": 2, "channels": [6, 4]}}
    assert a.cfg == {"earlier": True} and res.samplerate == 10.0
    s, t = CD.make_pair(1)
    t.freq, t.taper = np.arange(3) * 5.0, np.array(["x", "y"])
    res = spy.concat(s, t)
    assert list(res.freq) == [0.0, 10.0, 20.0] and list(res.taper) == ["t0", "t1"]
    assert np.array_equal(res.trialdefinition, [[0, 5, -2], [5, 9, -1], [9, 14, -2]])


def test_labels(on_emulator):
    a, b = CD.make_pair(0)
    assert list(spy.concat(b, a).channel) == [f"b{i}" for i in range(4)] + [f"a{i}" for i in range(6)]
    b.channel = np.array(["b0", "a3", "b2", "b3"])                                # a clash: the constructor's defaults
    res = CD.check_frontend([a, b], [a, b])
    assert list(res.channel) == ["channel%02d" % i for i in range(1, 11)]
    assert list(spy.concat(a, a).channel) == ["channel%02d" % i for i in range(1, 13)]
    s, t = CD.make_pair(1)
    assert list(spy.concat(s, t).channel) == [f"a{i}" for i in range(6)] + [f"b{i}" for i in range(4)]
    assert spy.concat(s, s).channel is None
    t.channel = None
    assert spy.concat(s, t).channel is None
    x, y = CD.make_pair(3)
    y.channel = np.array(["a0", "q", "r", "s"])
    assert spy.concat(x, y).channel is None
    x.avg = np.zeros((9, 6))
    assert spy.concat(x, CD.make_pair(3)[1]).avg is None


def test_checks(on_emulator):
    a, b = CD.make_pair(0)
    spike = spy.SpikeData(np.array([[1, 0, 0], [5, 1, 0]]), samplerate=10.0, trialdefinition=[[0, 10, 0]])
    for bad in ((a, spike), (spike, a), (a, b.data), (a.data, b), (a, b, None)):
        with pytest.raises(SPYTypeError, match="continuous data type"):
            spy.concat(*bad)
    for bad in ((a, spy.AnalogData()), (spy.AnalogData(), b), (a, b, spy.AnalogData())):
        with pytest.raises(SPYValueError, match="non-empty Syncopy data object"):
            spy.concat(*bad)
    s, t = CD.make_pair(1)
    m, _ = CD.make_pair(2)
    tl, _ = CD.make_pair(3)
    for bad in ((a, s), (s, m), (a, tl), (a, b, tl)):
        with pytest.raises(SPYValueError, match="objects with equal dimensional layout"):
            spy.concat(*bad)
    with pytest.raises(SPYValueError, match="object which has a `freq` dimension"):
        spy.concat(a, b, dim="freq")
    for dim in ("time", "taper", "freq"):
        with pytest.raises(NotImplementedError, match="Only `channel` concatenation supported atm"):
            spy.concat(s, t, dim=dim)
    with pytest.raises(NotImplementedError, match="Only `channel` concatenation supported atm"):
        spy.concat(a, b, dim="time")
    shorter = spy.AnalogData(b.data, samplerate=10.0, trialdefinition=b.trialdefinition[:3])
    more_rows = spy.AnalogData(np.concatenate([b.data, b.data[:1]]), samplerate=10.0, trialdefinition=b.trialdefinition)
    other_length = spy.AnalogData(b.data, samplerate=10.0, trialdefinition=[[3, 12, 0], [12, 24, 0], [25, 33, 0], [33, 43, 0]])
    freqs = spy.SpectralData(t.data[:, :, :2], samplerate=10.0, trialdefinition=t.trialdefinition)
    for bad in ((a, shorter), (a, more_rows), (a, other_length), (a, b, other_length), (s, freqs)):
        with pytest.raises(SPYValueError, match="objects with matching shapes"):
            spy.concat(*bad)
    with pytest.raises(SPYValueError, match="at most 8 objects"):
        spy.concat(*([a] * 9))
    assert spy.concat(*([a] * 8)).data.shape == (39, 48)


def test_cross_spectra_have_no_channel_dimension():
    import select_drive as SD
    c = SD.make("CrossSpectralData")
    with pytest.raises(SPYValueError, match="object which has a `channel` dimension"):
        spy.concat(c, c)
    with pytest.raises(NotImplementedError):
        spy.concat(c, c, dim="channel_i")


def test_deviations(on_emulator):
    a, b = CD.make_pair(0)
    flipped = [spy.AnalogData(np.ascontiguousarray(o.data.T), samplerate=10.0, trialdefinition=o.trialdefinition,
                              dimord=["channel", "time"]) for o in (a, b)]
    with pytest.raises(SPYValueError, match="data with time as its first dimension"):
        spy.concat(*flipped)
    wide = spy.AnalogData(b.data.astype(np.float64), samplerate=10.0, trialdefinition=b.trialdefinition)
    with pytest.raises(SPYValueError, match="float32 and float64"):
        spy.concat(a, wide)
    with pytest.raises(SPYValueError, match="float64 and float32"):
        spy.concat(wide, a)
    ints = spy.AnalogData(np.zeros(b.data.shape, dtype=np.int32), samplerate=10.0, trialdefinition=b.trialdefinition)
    with pytest.raises(SPYTypeError, match="float32, float64, complex64 or complex128"):
        spy.concat(ints, ints)
    b.selectdata({"trials": [0, 1, 2, 3], "channel": [0, 1]})
    with pytest.raises(SPYValueError, match="make the selection a new object with `spy.selectdata` first"):
        spy.concat(a, b)
    b.selectdata(None)
    assert spy.concat(a, b).data.shape == (39, 10)
