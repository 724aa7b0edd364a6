"""Operator arithmetic on data objects (syncopy_amd/datatype/arithmetic.py, csrc/arith.hip) without a GPU: the checks,
warnings and type rules of the front end, the result objects, and the library's own launcher and kernels at their
dispatch edges through the CPU emulation (tests/emu/arith_emu.cpp)."""
import warnings

import numpy as np
import pytest

import arith_drive as AD
import arith_oracle as AO
import build_emu
import syncopy_amd as spy
from syncopy_amd.datatype import Selection, arithmetic as A
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError

DT = {"f4": np.float32, "f8": np.float64, "c8": np.complex64, "c16": np.complex128}


@pytest.fixture(scope="module")
def emu():
    return AD.emu()


@pytest.fixture
def on_emulator(emu, monkeypatch):
    """the operators of the data classes, computed by the emulated library with two workgroups per launch"""
    monkeypatch.setattr(A, "_run", AD.emu_run(emu.few))


def _values(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def analog(dtype=np.float32, nchan=4, lengths=(5, 3, 6), seed=0):
    at, trl = 1, []
    for n in lengths:
        trl.append([at, at + n, -2])
        at += n + 1
    return spy.AnalogData(_values((at + 1, nchan), dtype, seed), samplerate=10.0, trialdefinition=trl)


def spectral(dtype=np.complex64, seed=0):
    s = spy.SpectralData(_values((12, 2, 3, 4), dtype, seed), samplerate=10.0,
                         trialdefinition=[[0, 4, -1], [4, 8, -1], [8, 12, -1]])
    s.freq, s.taper, s.channel = np.arange(3.0), np.array(["a", "b"]), np.array(["c0", "c1", "c2", "c3"])
    return s


def cross(dtype=np.complex64, seed=0):
    c = spy.CrossSpectralData(_values((6, 3, 2, 2), dtype, seed), samplerate=10.0,
                              trialdefinition=[[0, 2, 0], [2, 4, 0], [4, 6, 0]])
    c.freq, c.channel_i, c.channel_j = np.arange(3.0), np.array(["a", "b"]), np.array(["a", "b"])
    return c


def timelock(dtype=np.float32, seed=0):
    return spy.TimeLockData(_values((12, 4), dtype, seed), samplerate=10.0,
                            trialdefinition=[[0, 4, -1], [4, 8, -1], [8, 12, -1]], channel=["c0", "c1", "c2", "c3"])


MAKERS = {"AnalogData": analog, "SpectralData": spectral, "CrossSpectralData": cross, "TimeLockData": timelock}


# ---- the front end: errors, warnings, types -----------------------------------------------------------------------------
def test_operators_exist_and_compute(on_emulator):
    """`data + 1` raised TypeError before there were operators"""
    x = analog()
    res = x + 1
    assert isinstance(res, spy.AnalogData) and res.data.dtype == np.float32
    AD.assert_identical(res.data, AO.arith(x, 1, "+"))
    for cls in (spy.AnalogData, spy.SpectralData, spy.CrossSpectralData, spy.TimeLockData):
        for name in ("__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__rtruediv__",
                     "__pow__"):
            assert callable(getattr(cls, name))
        assert not hasattr(cls, "__rpow__")
        assert cls.__eq__ is object.__eq__ and cls.__hash__ is object.__hash__


def test_base_object_errors():
    spikes = spy.SpikeData(np.array([[1, 0, 0], [3, 1, 0]]), samplerate=10.0, trialdefinition=[[0, 5, 0]])
    with pytest.raises(SPYTypeError, match="Wrong type of `base`: expected `AnalogData`, `SpectralData` or `CrossSpectralData`"):
        spikes + 1
    with pytest.raises(SPYTypeError, match="of `base`"):
        2 * spikes
    with pytest.raises(SPYValueError, match="Invalid value of `base`: 'empty object'; expected non-empty Syncopy data object"):
        spy.AnalogData() + 1
    for dtype in (np.int16, np.int64, np.float16):
        x = spy.AnalogData(np.ones((4, 2), dtype=dtype), samplerate=1.0)
        with pytest.raises(SPYTypeError, match="expected float32, float64, complex64 or complex128 data"):
            x * 2


@pytest.mark.parametrize("bad", [True, np.bool_(False), "a", None, (1, 2), {"a": 1}])
def test_operand_type_errors(bad):
    with pytest.raises(SPYTypeError, match="Wrong type of `operand`: expected Syncopy object, scalar or array-like"):
        analog() + bad
    with pytest.raises(SPYTypeError, match="of `operand`"):
        A._process_operator(bad, analog(), "-")


def test_scalar_errors():
    x = analog()
    for s in (np.inf, -np.inf, np.float32(np.inf), complex(np.inf, 0)):
        with pytest.raises(SPYValueError, match="expected finite scalar"):
            x + s
        with pytest.raises(SPYValueError, match="expected finite scalar"):
            s - x
    for s in (0, 0.0, np.float32(0), 0j):
        with pytest.raises(SPYValueError, match="Invalid value of `operand`: '.*'; expected non-zero scalar for division"):
            x / s
    assert A._plan(0, x, "/").op == "rdiv"                                  # 0 / data: only a zero DIVISOR raises
    assert A._plan(x, 0, "*").op == "mul"


def test_array_errors():
    x = analog(lengths=(5, 3))
    with pytest.raises(SPYValueError, match=r"expected array compatible to trial shape \(5, 4\)"):
        x + np.ones(3)
    with pytest.raises(SPYValueError, match=r"'array with shape \(5, 4\)'; expected array compatible to trial shape \(3, 4\)"):
        x + np.ones((5, 4))                                                   # fits the first trial only
    with pytest.raises(SPYValueError, match=r"array with shape \(2, 1, 4\)"):
        x * np.ones((2, 1, 4))                                                # would enlarge the trials
    with pytest.raises(SPYValueError, match=r"array with shape \(2, 1, 1\)"):
        [[[1.0]], [[2.0]]] * x
    with pytest.raises(SPYTypeError, match="of `operand`: expected array of numbers"):
        x + np.array(["a", "b", "c", "d"])
    with pytest.raises(SPYTypeError, match="of `operand`"):
        x + [True, False, True, True]
    assert A._plan(x, [1, 2, 3, 4], "+").array.dtype == np.float64            # np.array(list) is int64: NumPy promotes


def test_object_operand_errors():
    x = analog()
    with pytest.raises(SPYTypeError, match="of `operand`: expected Syncopy AnalogData object"):
        x + timelock()
    with pytest.raises(SPYTypeError, match="of `operand`"):
        spectral() - cross()
    with pytest.raises(SPYValueError, match="of `operand`: 'empty object'; expected non-empty Syncopy data object"):
        x + spy.AnalogData()
    y = analog()
    y.samplerate = 20.0
    with pytest.raises(SPYValueError, match="Syncopy object with samplerates 10.0 and 20.0, respectively"):
        x - y
    t = spy.AnalogData(np.ones((4, 8), dtype=np.float32), samplerate=10.0, dimord=["channel", "time"],
                       trialdefinition=[[0, 8, 0]])
    with pytest.raises(SPYValueError, match="of `operand`.*dimord"):
        x + t
    with pytest.raises(SPYValueError, match=r"'Syncopy object with 2 trials \(selected\)'; expected Syncopy object with same "
                                            r"number of trials \(selected\)"):
        x + analog(lengths=(5, 3))
    with pytest.raises(SPYValueError, match=r"expected Syncopy object \(selection\) of compatible shapes \[\(5, 4\), \(3, 4\), "
                                            r"\(6, 4\)\]"):
        x + analog(lengths=(5, 4, 6))
    with pytest.raises(SPYValueError, match="of compatible shapes"):
        x + analog(nchan=3)
    with pytest.raises(SPYTypeError, match=r"expected Syncopy data object of same numerical type \(real/complex\)"):
        x + analog(np.complex64)
    with pytest.raises(SPYTypeError, match="float32, float64, complex64 or complex128 data"):
        x + spy.AnalogData(np.ones((17, 4), dtype=np.int32), samplerate=10.0, trialdefinition=x.trialdefinition)


def test_operand_selection_rules(on_emulator):
    x, y = analog(lengths=(4, 4, 4)), analog(lengths=(4, 4, 4), seed=1)
    x.selectdata({"trials": [2, 0], "channel": [3, 1]})
    for wild in ({"trials": [2, 0], "channel": [1, 3]}, {"trials": [0, 0], "channel": [1, 3]},
                 {"trials": [0, 2], "channel": [3, 1]}, {"trials": [0, 2], "channel": [1, 1]}):
        y.selectdata(wild)
        with pytest.warns(UserWarning, match="Found existing in-place selection in operand"):
            with pytest.raises(SPYValueError, match="expected Syncopy object with ordered unreverberated subset selection"):
                x - y
    y.selectdata({"trials": [0, 2], "channel": [1, 3]})
    with pytest.warns(UserWarning, match="Shapes and trial counts of base and operand objects have to match up!"):
        res = x - y
    AD.assert_identical(res.data, AO.arith(x, y, "-"))
    assert res.cfg["operand selection"] == {"trials": [0, 2], "channel": [1, 3]}
    assert y.selection is not None and x.selection.select == {"trials": [2, 0], "channel": [3, 1]}


def test_real_complex_mismatch_warns(on_emulator):
    x, z = analog(), analog(np.complex64)
    with pytest.warns(UserWarning, match=r"Syncopy <\+> WARNING: Operand is scalar of different mathematical type \(real/complex\)"):
        res = x + (1 + 2j)
    assert res.data.dtype == np.complex64                                     # computed in the promoted type
    AD.assert_identical(res.data, AO.arith(x, 1 + 2j, "+"))
    with pytest.warns(UserWarning, match="Operand is scalar of different mathematical type"):
        res = z * 2.0
    AD.assert_identical(res.data, AO.arith(z, 2.0, "*"))
    with pytest.warns(UserWarning, match=r"<-> WARNING: Operand is array of different mathematical type"):
        res = x - np.array([1j, 2, 3, 4])
    assert res.data.dtype == np.complex128
    AD.assert_identical(res.data, AO.arith(x, np.array([1j, 2, 3, 4]), "-"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x + 1.0, z + 1j, x * np.ones(4), z * np.ones(4, dtype=np.complex64)   # no mismatch, no warning


@pytest.mark.filterwarnings("ignore:Syncopy")
@pytest.mark.parametrize("name", ["f4", "f8", "c8", "c16"])
def test_result_dtype_is_numpys(name, on_emulator):
    """np.result_type(<trial dtypes>, operand), called the way the reference calls it (NumPy >= 2: a Python scalar is weak)"""
    x = analog(DT[name])
    operands = [1, 2.5, np.float32(2.5), np.float64(2.5), np.int64(3), np.ones(4, dtype=np.float32), np.ones(4),
                np.arange(1, 5), np.ones(4, dtype=np.float16)]
    if np.dtype(DT[name]).kind == "c":
        operands += [1 + 1j, np.complex64(1j), np.complex128(1j), np.ones(4, dtype=np.complex128)]
    for s in operands:
        want = np.result_type(x.data.dtype, s if np.isscalar(s) else s.dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = x * s
        assert res.data.dtype == want, (name, type(s), res.data.dtype, want)
        AD.assert_identical(res.data, AO.arith(x, s, "*")) if want.kind != "c" else None
    if name == "f4":
        assert (x + 2.5).data.dtype == np.float32 and (x + np.float64(2.5)).data.dtype == np.float64
    with pytest.raises(SPYTypeError, match="of `result`"):
        x + np.ones(4, dtype=np.longdouble)
    for other in ("f4", "f8") if np.dtype(DT[name]).kind == "f" else ("c8", "c16"):
        res = x - analog(DT[other], seed=3)
        assert res.data.dtype == np.result_type(DT[name], DT[other])
        AD.assert_identical(res.data, AO.arith(x, analog(DT[other], seed=3), "-"))


def test_complex_power_is_refused():
    x, z = analog(), analog(np.complex64)
    for base, e in ((z, 2), (z, 0.5), (x, 2j), (x, np.array([1j, 1, 1, 1])), (z, z), (z, np.ones(4))):
        with pytest.raises(NotImplementedError, match="complex base or a complex exponent"):
            base ** e
    with pytest.raises(TypeError):
        2 ** x                                                                # __rpow__ stays undefined


# ---- result objects -----------------------------------------------------------------------------------------------------
SELECT = {"trials": [2, 0, 2], "channel": [3, 1], "latency": [0.0, 0.15]}


@pytest.mark.filterwarnings("ignore:Syncopy")
@pytest.mark.parametrize("cls", list(MAKERS))
@pytest.mark.parametrize("selected", [False, True])
def test_result_metadata(cls, selected, on_emulator):
    x = MAKERS[cls]()
    if cls == "AnalogData":
        x.channel = np.array(["c0", "c1", "c2", "c3"])
    sel = None
    if selected:
        sel = dict(SELECT) if cls != "CrossSpectralData" else {"trials": [2, 0, 2]}
        x.selection = Selection(x, sel)
    before = x.selection
    res = 2.0 - x
    assert type(res) is type(x) and res.dimord == x.dimord and res.samplerate == x.samplerate
    assert x.selection is before                                              # the base's selection survives the call
    want = AO.arith(x, 2.0, "-", reflected=True)
    AD.assert_identical(res.data, want)
    n = [t.shape[0] for t in res.trials]
    if selected and cls != "CrossSpectralData":
        assert np.array_equal(res.trialdefinition, x.selection.trialdefinition)
        assert list(res.channel) == ["c3", "c1"] and res.data.shape[-1] == 2
        assert n[0] == n[2] and res.trialdefinition[0, 2] == x.selection.trialdefinition[0, 2]
    else:
        ids = [2, 0, 2] if selected else [0, 1, 2]
        assert np.array_equal(res.trialdefinition[:, 2:], x.trialdefinition[ids, 2:])
        if cls != "CrossSpectralData":
            assert list(res.channel) == ["c0", "c1", "c2", "c3"]
    assert np.array_equal(res.trialdefinition[:, 1] - res.trialdefinition[:, 0], n)
    assert res.trialdefinition[0, 0] == 0 and res.trialdefinition[-1, 1] == res.data.shape[0]   # stacked, nothing else
    for prop in ("freq", "taper", "channel_i", "channel_j"):
        if getattr(x, prop, None) is not None:
            assert np.array_equal(getattr(res, prop), getattr(x, prop))
    if cls == "TimeLockData":
        assert res.avg is None and res.var is None and res.cov is None
    assert res.cfg == {"operator": "-", "base": cls, "base selection": sel, "operand": "float", "operand selection": None}


def test_rows_outside_the_trials_do_not_appear(on_emulator):
    x = analog(lengths=(5, 3, 6))                                             # a gap row in front of every trial
    res = x * 3
    assert res.data.shape[0] == 14 and x.data.shape[0] == 19
    assert np.array_equal(res.trialdefinition[:, :2], [[0, 5], [5, 8], [8, 14]])
    AD.assert_identical(res.data, np.concatenate([t * np.float32(3) for t in x.trials]))


# ---- the launcher and the kernels at their dispatch edges (two workgroups per launch) ---------------------------------------
def _stacked(trl):
    n = (trl[:, 1] - trl[:, 0]).astype(np.int64)
    starts = np.concatenate(([0], np.cumsum(n)))
    return n, starts


@pytest.mark.parametrize("nchan", AD.EDGE_CHANNELS)
@pytest.mark.parametrize("gap", [0, 1])
def test_edge_lengths_and_odd_starts(nchan, gap, emu):
    """trials of 1, 3, 4, 5 and 257 samples in ONE launch, starting anywhere: scalar, array and full-tensor operands"""
    x, trl = AD.edge_analog(nchan, gap=gap)
    y, _ = AD.edge_analog(nchan, seed=1, gap=gap)
    n, starts = _stacked(trl)
    desc = np.stack([starts[:-1], trl[:, 0], trl[:, 0], n], axis=1)
    trials = [x[int(a):int(b)] for a, b in trl[:, :2]]
    w = np.arange(1, nchan + 1, dtype=np.float32)
    build_emu.launches(emu)
    for ctx in (emu.ctx, emu.few):
        out = np.full((starts[-1], nchan), np.nan, dtype=np.float32)
        assert AD.emu_arith("add", x, desc, out, scalar=1.5, ctx=ctx) == 0
        AD.assert_identical(out, np.concatenate(trials) + np.float32(1.5))
        assert AD.emu_arith("mul", x, desc, out, array=w, ctx=ctx) == 0
        AD.assert_identical(out, np.concatenate([t * w for t in trials]))
        assert AD.emu_arith("rsub", x, desc, out, operand=None, array=w.reshape(1, nchan), ctx=ctx) == 0
        AD.assert_identical(out, np.concatenate([w - t for t in trials]))
        assert AD.emu_arith("sub", x, desc, out, operand=y, ctx=ctx) == 0
        AD.assert_identical(out, np.concatenate(trials) - np.concatenate([y[int(a):int(b)] for a, b in trl[:, :2]]))
    grids = build_emu.launches(emu)[:, 0]
    total = int(starts[-1]) * nchan
    vec = nchan == 4                            # rows of 16 bytes: every start on a boundary; else hardly any, gap or not
    assert list(grids[:4]) == [(total // 4 + 255) // 256 if vec else (total + 255) // 256] * 4 and list(grids[4:]) == [2] * 4


def test_vector_items_with_a_short_last_one(emu):
    """aligned starts whose last trial ends inside an item: the 16-byte path with its element-wise end"""
    x = _values((523, 3), np.float32)
    desc = np.array([[0, 8, 0, 4], [4, 100, 0, 256], [260, 0, 0, 1]])          # starts at elements 24, 300, 0: all % 4 == 0
    out = np.full((261, 3), np.nan, dtype=np.float32)
    build_emu.launches(emu)
    assert AD.emu_arith("rdiv", x, desc, out, scalar=2.0) == 0
    assert build_emu.launches(emu)[0, 0] == 1                                  # 196 items of 4 (783 elements would be 4 blocks)
    AD.assert_identical(out, np.float32(2) / np.concatenate([x[8:12], x[100:356], x[0:1]]))


@pytest.mark.parametrize("shape", [(5, 1, 1, 1), (1, 2, 1, 1), (1, 1, 3, 1), (1, 1, 1, 4), (1, 1, 1, 1), (5, 2, 3, 4),
                                   (3, 4), (4,), (2, 1, 4), ()])
def test_array_broadcast_along_every_axis(shape, emu):
    x = _values((17, 2, 3, 4), np.float32)
    w = _values(shape, np.float32, seed=2)
    desc = np.array([[0, 11, 0, 5], [5, 0, 0, 5], [10, 6, 0, 5]])             # 5 samples each, overlapping base rows
    out = np.empty((15, 2, 3, 4), dtype=np.float32)
    for ctx in (emu.ctx, emu.few):
        out[:] = np.nan
        assert AD.emu_arith("mul", x, desc, out, array=w, ctx=ctx) == 0
        AD.assert_identical(out, np.concatenate([x[11:16] * w, x[0:5] * w, x[6:11] * w]))
    z = _values((17, 2, 3, 4), np.complex64)
    wz = w.astype(np.complex64)
    outz = np.empty((15, 2, 3, 4), dtype=np.complex64)
    assert AD.emu_arith("add", z, desc, outz, array=wz, ctx=emu.few) == 0
    AD.assert_identical(outz, np.concatenate([z[11:16] + wz, z[0:5] + wz, z[6:11] + wz]))


def test_repeated_and_reordered_trials_with_channels(emu):
    x = _values((40, 2, 5), np.float64)
    y = _values((40, 2, 3), np.float64, seed=1)
    rows = [(30, 37), (3, 4), (30, 37), (10, 13), (3, 4)]
    n = np.array([b - a for a, b in rows])
    starts = np.concatenate(([0], np.cumsum(n)))
    chan = [4, 0, 4]
    desc = np.stack([starts[:-1], [a for a, _ in rows], [a for a, _ in rows], n], axis=1)
    out = np.full((starts[-1], 2, 3), np.nan)
    assert AD.emu_arith("div", x, desc, out, operand=y, chan=chan, ctx=emu.few) == 0
    AD.assert_identical(out, np.concatenate([x[a:b][..., chan] / y[a:b] for a, b in rows]))
    assert AD.emu_arith("copy", x, desc, out, chan=chan, ctx=emu.few) == 0
    AD.assert_identical(out, np.concatenate([x[a:b][..., chan] for a, b in rows]))


@pytest.mark.parametrize("pair", AD.PAIRS, ids=["->".join(p) for p in AD.PAIRS])
def test_type_pairs(pair, emu):
    """the base is converted in the load: all nine base -> result pairs, every operand mode, vector and scalar instance"""
    a_t, o_t = DT[pair[0]], DT[pair[1]]
    for nchan in (4, 3):
        x = _values((20, nchan), a_t)
        y = _values((20, nchan), o_t, seed=1)
        w = _values((nchan,), o_t, seed=2)
        s = o_t(1.25 - 0.5j) if np.dtype(o_t).kind == "c" else o_t(1.25)
        desc = np.array([[0, 12, 4, 8], [8, 1, 13, 7]])
        out = np.empty((15, nchan), dtype=o_t)
        xs, ys = np.concatenate([x[12:20], x[1:8]]).astype(o_t), np.concatenate([y[4:12], y[13:20]])
        def same(got, want, what):                  # complex quotients: the parity tests below say how close they must be
            if what[0] in ("div", "rdiv") and np.dtype(o_t).kind == "c":
                assert got.dtype == want.dtype and np.allclose(got, want, rtol=8 * AD.unit_roundoff(o_t), atol=0), what
            else:
                AD.assert_identical(got, want, what)
        for op, f in (("add", np.add), ("sub", np.subtract), ("div", np.divide)):
            assert AD.emu_arith(op, x, desc, out, scalar=s, ctx=emu.few) == 0
            same(out, f(xs, s), (op, "scalar"))
            assert AD.emu_arith(op, x, desc, out, array=w, ctx=emu.few) == 0
            same(out, f(xs, w), (op, "array"))
            assert AD.emu_arith(op, x, desc, out, operand=y, ctx=emu.few) == 0
            same(out, f(xs, ys), (op, "object"))
        for op, f in (("rsub", np.subtract), ("rdiv", np.divide)):
            assert AD.emu_arith(op, x, desc, out, scalar=s, ctx=emu.few) == 0
            same(out, f(s, xs), (op, "scalar"))
            assert AD.emu_arith(op, x, desc, out, array=w, ctx=emu.few) == 0
            same(out, f(w, xs), (op, "array"))
        assert AD.emu_arith("copy", x, desc, out, ctx=emu.few) == 0
        AD.assert_identical(out, xs)


def test_launcher_refuses_what_does_not_fit(emu):
    x, out = _values((10, 4), np.float32), np.zeros((6, 4), dtype=np.float32)
    ok = np.array([[0, 2, 0, 3], [3, 7, 0, 3]])
    assert AD.emu_arith("add", x, ok, out, scalar=1.0) == 0
    for bad in ([[0, 2, 0, 3], [3, 8, 0, 3]],          # base rows 8 .. 11 of 10
                [[0, 2, 0, 3], [3, 7, 0, 4]],          # output rows 3 .. 7 of 6
                [[0, 2, 0, 3], [4, 7, 0, 2]],          # a hole in the output
                [[0, -1, 0, 3]], [[0, 2, 0, -3]]):
        assert AD.emu_arith("add", x, np.array(bad), out, scalar=1.0) == -1
    assert AD.emu_arith("sub", x, ok, out, operand=np.zeros((2, 4), dtype=np.float32)) == -1      # operand rows 0 .. 3 of 2
    assert AD.emu_arith("add", x, ok, out[:, :2].copy(), scalar=1.0, chan=[0, 4]) == -1           # channel 4 of 4
    assert AD.emu_arith("pow", _values((10, 4), np.complex64), ok, out.astype(np.complex64), scalar=2.0) == -1
    assert AD.emu_arith("rsub", x, ok, out, operand=x.copy()) == -1                                # not provided
    assert AD.emu_arith("add", x.astype(np.float64), ok, out, scalar=1.0) == -1                    # float64 -> float32


# ---- parity with NumPy (the emulator runs the kernels' own arithmetic on the host) --------------------------------------------
def _apply_on(ctx):
    run = AD.emu_run(ctx)

    def apply(x, operand, operator, reflected):
        x = np.asarray(x)
        nchan = 5 if x.size % 5 == 0 else 1
        obj = spy.AnalogData(x.reshape(-1, nchan), samplerate=1.0)
        if isinstance(operand, np.ndarray):             # a second object; reflected: an array of the one trial's shape
            operand = operand.reshape(-1, nchan) if reflected else spy.AnalogData(operand.reshape(-1, nchan), samplerate=1.0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plan = A._plan(operand, obj, operator) if reflected else A._plan(obj, operand, operator)
            out = A._new_object(plan)
            run(plan, out)
        return out.data.reshape(x.shape)
    return apply


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_real(dtype, emu):
    AD.check_real_exact(_apply_on(emu.few), dtype)
    AD.check_power_fast_paths(_apply_on(emu.few), dtype)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_parity_complex(dtype, emu):
    AD.check_complex(_apply_on(emu.few), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_parity_against_the_wider_type(dtype, emu):
    why = AD.needs_longdouble(dtype)
    if why:
        pytest.skip(why)
    assert np.finfo(np.longdouble).nmant >= 63 or np.dtype(dtype).itemsize <= 8
    if np.dtype(dtype).kind == "c":
        AD.check_complex_division(_apply_on(emu.few), dtype)
    else:
        AD.check_power(_apply_on(emu.few), dtype)
