"""Operator arithmetic on data objects on the device: the kernels of syncopy_amd/csrc/arith_kernel.h through the operators
of the data classes, from a device copy and through chunked uploads, against NumPy applied per trial
(tests/arith_oracle.py), at the shapes of tests/test_arith.py, one case beyond the cap on workgroups and one chain that
never touches the host.  The criteria are those of tests/arith_drive.py; the figures they print are in DESIGN.md
section 8."""
import warnings

import numpy as np
import pytest

import arith_drive as AD
import arith_oracle as AO
import syncopy_amd as spy
from syncopy_amd.datatype import Selection, arithmetic as A

pytestmark = pytest.mark.gpu

DT = {"f4": np.float32, "f8": np.float64, "c8": np.complex64, "c16": np.complex128}


def apply(x, operand, operator, reflected):
    """one AnalogData trial of 5 (or 1) channels against a scalar, a second object or, reflected, an array"""
    x = np.asarray(x)
    nchan = 5 if x.size % 5 == 0 else 1
    obj = spy.AnalogData(x.reshape(-1, nchan), samplerate=1.0)
    if isinstance(operand, np.ndarray):
        operand = operand.reshape(-1, nchan) if reflected else spy.AnalogData(operand.reshape(-1, nchan), samplerate=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = A._process_operator(operand, obj, operator) if reflected else A._process_operator(obj, operand, operator)
    return res.data.reshape(x.shape)


def _resident(x):
    """x with its float32 / complex64 matrix on the device and no host copy, as a front end leaves a result"""
    import torch
    out = spy.AnalogData(None, samplerate=x.samplerate, channel=x.channel)
    out.trialdefinition = x.trialdefinition
    out.adopt_device_result(torch.from_numpy(np.ascontiguousarray(x.data)).cuda())
    return out


@pytest.mark.parametrize("nchan", AD.EDGE_CHANNELS)
@pytest.mark.parametrize("where", ["host", "chunks", "device"])
def test_edge_lengths_and_odd_starts(nchan, where, monkeypatch):
    """trials of 1, 3, 4, 5 and 257 samples behind a gap row each: one launch from the device copy, one per chunk (of two
    short trials, or one long one) from the host"""
    data, trl = AD.edge_analog(nchan)
    other, _ = AD.edge_analog(nchan, seed=1)
    x = spy.AnalogData(data, samplerate=100.0, trialdefinition=trl)
    y = spy.AnalogData(other, samplerate=100.0, trialdefinition=trl)
    if where == "chunks":
        monkeypatch.setattr(A, "CHUNK_BYTES", 8 * nchan * 4)
    xs, ys = (_resident(x), _resident(y)) if where == "device" else (x, y)
    w = np.arange(1, nchan + 1, dtype=np.float32)
    AD.assert_identical((xs + 1.5).data, AO.arith(x, 1.5, "+"))
    AD.assert_identical((xs * w).data, AO.arith(x, w, "*"))
    AD.assert_identical((w - xs).data, AO.arith(x, w, "-", reflected=True))
    AD.assert_identical((2 / xs).data, AO.arith(x, 2, "/", reflected=True))
    AD.assert_identical((xs - ys).data, AO.arith(x, y, "-"))
    AD.assert_identical((xs / np.float64(3)).data, AO.arith(x, np.float64(3), "/"))
    if where == "device":
        assert xs._data is None and ys._data is None


@pytest.mark.parametrize("shape", [(5, 1, 1, 1), (1, 2, 1, 1), (1, 1, 3, 1), (1, 1, 1, 4), (1, 1, 1, 1), (5, 2, 3, 4),
                                   (3, 4), (4,)])
def test_array_broadcast_along_every_axis(shape):
    rng = np.random.default_rng(0)
    s = spy.SpectralData(rng.standard_normal((15, 2, 3, 4)).astype(np.float32), samplerate=10.0,
                         trialdefinition=[[0, 5, 0], [5, 10, 0], [10, 15, 0]])
    s.channel = np.array(["a", "b", "c", "d"])
    w = rng.standard_normal(shape).astype(np.float32)
    AD.assert_identical((s * w).data, AO.arith(s, w, "*"))
    AD.assert_identical((w / s).data, AO.arith(s, w, "/", reflected=True))
    s.selection = Selection(s, {"trials": [2, 0, 2]})
    AD.assert_identical((s + w).data, AO.arith(s, w, "+"))


@pytest.mark.parametrize("where", ["host", "device"])
def test_selection_with_repeats_channels_and_latency(where):
    rng = np.random.default_rng(1)
    trl = [[0, 9, -2], [9, 20, -3], [20, 27, -2]]
    x = spy.AnalogData(rng.standard_normal((27, 5)).astype(np.float32), samplerate=10.0, trialdefinition=trl)
    y = spy.AnalogData(rng.standard_normal((27, 5)).astype(np.float32), samplerate=10.0, trialdefinition=trl)
    xs, ys = (_resident(x), _resident(y)) if where == "device" else (x, y)
    select = {"trials": [2, 0, 2], "channel": [3, 1], "latency": [0.0, 0.35]}
    for obj in (x, xs):
        obj.selectdata(select)
    for obj in (y, ys):
        obj.selectdata({"trials": [0, 1, 2], "channel": [0, 4], "latency": [-0.1, 0.25]})
    with pytest.warns(UserWarning, match="Found existing in-place selection in operand"):
        res = xs - ys
    AD.assert_identical(res.data, AO.arith(x, y, "-"))
    assert list(res.channel) == list(np.array(x.channel)[[3, 1]]) and np.array_equal(res.trialdefinition,
                                                                                    x.selection.trialdefinition)
    assert xs.selection.select == select
    AD.assert_identical((xs ** 2).data, AO.arith(x, 2, "**"))
    AD.assert_identical((1.5 - xs).data, AO.arith(x, 1.5, "-", reflected=True))


@pytest.mark.parametrize("pair", AD.PAIRS, ids=["->".join(p) for p in AD.PAIRS])
def test_type_pairs(pair):
    """every base -> result pair, reached the way a user reaches it: by the operand's type"""
    a_t, o_t = DT[pair[0]], DT[pair[1]]
    rng = np.random.default_rng(2)

    def values(dtype, n=14):
        v = rng.standard_normal((n, 3))
        return (v + 1j * rng.standard_normal((n, 3)) if np.dtype(dtype).kind == "c" else v).astype(dtype)
    trl = [[1, 6, 0], [6, 14, 0]]
    x = spy.AnalogData(values(a_t), samplerate=1.0, trialdefinition=trl)
    s = o_t(1.25 - 0.5j) if np.dtype(o_t).kind == "c" else o_t(1.25)
    w = values(o_t, 1)[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for operand in (s, w):
            for op in "+-":
                res = A._process_operator(x, operand, op)
                AD.assert_identical(res.data, AO.arith(x, operand, op))
                AD.assert_identical(A._process_operator(operand, x, op).data, AO.arith(x, operand, op, reflected=True))
        if (np.dtype(a_t).kind == "c") == (np.dtype(o_t).kind == "c"):
            y = spy.AnalogData(values(o_t), samplerate=1.0, trialdefinition=trl)
            AD.assert_identical((x + y).data, AO.arith(x, y, "+"))
            AD.assert_identical((y - x).data, AO.arith(y, x, "-"))
    assert res.data.dtype == np.dtype(o_t)


def test_beyond_the_cap_on_workgroups():
    """4096 workgroups x 256 threads x 4 elements and 3 more (17 MB of float32): every workgroup walks more than one
    round of items, and the last item is short"""
    n = 4096 * 256 * 4 + 3
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32).reshape(n, 1)
    a = spy.AnalogData(x, samplerate=1.0)
    AD.assert_identical((a * 1.5).data, x * np.float32(1.5))
    b = _resident(a)
    AD.assert_identical((b - a).data, np.zeros_like(x))


def test_chain_stays_on_the_device():
    """(a - b) / 2.0 + w on resident data: NumPy's result, and no host copy of an input or an intermediate result"""
    rng = np.random.default_rng(4)
    trl = [[0, 300, -10], [300, 533, -10], [533, 900, 0]]
    xa, xb = (rng.standard_normal((900, 7)).astype(np.float32) for _ in range(2))
    a = _resident(spy.AnalogData(xa, samplerate=100.0, trialdefinition=trl))
    b = _resident(spy.AnalogData(xb, samplerate=100.0, trialdefinition=trl))
    w = rng.standard_normal(7).astype(np.float32)
    d = a - b
    e = d / 2.0
    res = e + w
    assert a._data is None and b._data is None and d._data is None and e._data is None and res._data is None
    AD.assert_identical(((a - b) / 2.0 + w).data, (xa - xb) / np.float32(2.0) + w)
    AD.assert_identical(res.data, (xa - xb) / np.float32(2.0) + w)
    assert a._data is None and b._data is None and d._data is None and e._data is None
    # a float64 result and a cross-spectrum stay resident too
    f = (a * np.float64(2)) - 1
    assert f._data is None and f.data_dtype == np.float64
    AD.assert_identical(f.data, xa * np.float64(2) - 1)
    c = spy.CrossSpectralData((rng.standard_normal((4, 3, 2, 2)) + 1j).astype(np.complex64), samplerate=10.0,
                              trialdefinition=[[0, 2, 0], [2, 4, 0]])
    g = (c + 1j) - c
    assert g._data is None and g._dev is not None
    AD.assert_identical(g.data, (c.data + np.complex64(1j)) - c.data)


def test_numpy_only_host():
    """the torch-free wrapper Device.arith over the same entry point"""
    from syncopy_amd import abi
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((20, 2, 5)).astype(np.float32), rng.standard_normal((20, 2, 3))
    trials = [[12, 20], [1, 8], [12, 20]]
    dev = abi.Device(0)
    try:
        got = dev.arith("rdiv", x, trials, 2.0)
        AD.assert_identical(got, np.float32(2) / np.concatenate([x[a:b] for a, b in trials]))
        got = dev.arith("mul", x, trials, y[0, 0], channels=[4, 0, 1])
        AD.assert_identical(got, np.concatenate([x[a:b][..., [4, 0, 1]] * y[0, 0] for a, b in trials]))
        got = dev.arith("sub", x, trials, y, operand_trials=[[0, 8], [8, 15], [0, 8]], channels=[4, 0, 1])
        want = [x[a:b][..., [4, 0, 1]] - y[c:d] for (a, b), (c, d) in zip(trials, [[0, 8], [8, 15], [0, 8]])]
        AD.assert_identical(got, np.concatenate(want))
    finally:
        dev.close()


# ---- parity with NumPy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_real(dtype):
    AD.check_real_exact(apply, dtype)
    AD.check_power_fast_paths(apply, dtype)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_parity_complex(dtype):
    AD.check_complex(apply, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_parity_against_the_wider_type(dtype):
    """complex / and real ** with an exponent that has no fast path: at most twice NumPy's own largest relative error,
    both measured against the exact result in the next wider type"""
    why = AD.needs_longdouble(dtype)
    if why:
        pytest.skip(why)
    assert np.finfo(np.longdouble).nmant >= 63 or np.dtype(dtype).itemsize <= 8
    if np.dtype(dtype).kind == "c":
        AD.check_complex_division(apply, dtype)
    else:
        AD.check_power(apply, dtype)
