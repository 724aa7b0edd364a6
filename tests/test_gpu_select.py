"""spy.selectdata, spy.copy and spy.redefinetrial on the device: the kernels of syncopy_amd/csrc/select_kernel.h at the
dispatch edges of tests/select_drive.py (element sizes, the 16-byte boundary, trial tables, index lists around the LDS
cap, a launch beyond the cap on workgroups), the four data classes end to end from host data, chunked host data and
resident data, chains that never touch the host, and the torch-free wrapper.  Every comparison is bit for bit against
NumPy indexing (tests/select_oracle.py); the lane width of every kernel case is asserted through the route shim."""
import numpy as np
import pytest

import select_drive as SD
import select_oracle as SO
import syncopy_amd as spy
from syncopy_amd.datatype import selectdata as S

pytestmark = pytest.mark.gpu


def gather(src, trials, axes, skew=0):
    """backend.select on a source that lies `skew` bytes into its allocation"""
    import torch
    from syncopy_amd import backend
    raw = torch.empty(src.nbytes + 16, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    raw[skew:skew + src.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1).view(np.uint8)))
    dev = raw[skew:skew + src.nbytes].view(torch.from_numpy(src[:0]).dtype).reshape(src.shape)
    desc = SD.table(trials)
    count = S.select_axes(src.shape[1:], axes)[3]
    out = torch.empty((int(desc[:, 2].sum()),) + tuple(int(c) for c in count[4 - src.ndim:]), dtype=dev.dtype, device="cuda")
    out.view(torch.uint8).fill_(0xAB)
    backend.select(dev, desc, out, axes)
    return backend.to_host(out), dev.data_ptr(), out.data_ptr()


def _resident(x):
    """x with its data on the device and no host copy, as a front end leaves a result"""
    import torch
    out = x.__class__(None, samplerate=x.samplerate, dimord=x.dimord)
    out.trialdefinition = x.trialdefinition
    for prop in ("freq", "taper", "channel", "channel_i", "channel_j"):
        if getattr(x, prop, None) is not None:
            setattr(out, prop, np.array(getattr(x, prop)))
    S._adopt(out, torch.from_numpy(np.ascontiguousarray(x.data)).cuda(), x.data.dtype)
    return out


@pytest.mark.parametrize("name", list(SD.DT))
def test_element_sizes(name):
    SD.check_element_sizes(gather, name)


def test_sixteen_byte_boundary():
    SD.check_boundary(gather)


def test_trials():
    SD.check_trials(gather)


def test_index_lists():
    SD.check_index_lists(gather)


def test_beyond_the_cap_on_workgroups():
    """4096 workgroups x 256 threads x 4 elements and 3 more (17 MB of float32): every workgroup walks more than one
    round.  The 3 odd elements keep the whole-row copy on element lanes; one element more, as rows of 4 channels, moves
    16 bytes per lane, and two of the 4 channels go through the axis arithmetic"""
    n = 4096 * 256 * 4 + 3
    x = np.random.default_rng(3).standard_normal(n + 1).astype(np.float32)
    a = spy.AnalogData(x[:n].reshape(n, 1), samplerate=1.0)
    SD.same_bits(spy.copy(_resident(a)).data, a.data)
    assert SD.route(4, n, (1,), [(0, n)], None).lane == 4
    m = 4096 * 256 + 1
    b = spy.AnalogData(x.reshape(m, 4), samplerate=1.0)
    SD.same_bits(spy.copy(_resident(b)).data, b.data)
    assert SD.route(4, m, (4,), [(0, m)], None).lane == 16
    SD.same_bits(spy.selectdata(b, channel=slice(2, 4)).data, b.data[:, 2:4])
    assert SD.route(4, m, (4,), [(0, m)], [(2, 2)]).mode == SD.AXES


@pytest.mark.parametrize("where", ["host", "chunks", "device"])
@pytest.mark.parametrize("case", range(len(SD.FRONT_CASES)), ids=[c[0] + str(i) for i, c in enumerate(SD.FRONT_CASES)])
def test_classes_end_to_end(case, where, monkeypatch):
    cls, kwargs = SD.FRONT_CASES[case]
    host = SD.make(cls)
    if where == "chunks":                                                     # two short trials, or one long one, at a time
        monkeypatch.setattr(S, "CHUNK_BYTES", 12 * int(np.prod(host.data.shape[1:])) * host.data.dtype.itemsize)
    obj = _resident(host) if where == "device" else host
    res = SD.check_frontend(obj, host, kwargs)
    if where == "device":
        assert obj._data is None
    assert res._pending is None                                               # (check_frontend has read the result)


@pytest.mark.parametrize("name", ["f8", "c16"])
def test_wide_types_end_to_end(name):
    for cls in ("AnalogData", "SpectralData"):
        host = SD.make(cls, SD.DT[name])
        SD.check_frontend(host, host, {"trials": [2, 0], "channel": [4, 1]})
        SD.check_frontend(_resident(host), host, {"trials": [1], "channel": slice(1, 5), "latency": [-0.1, 0.1]})


def test_a_trial_without_rows_and_a_window_of_one_row():
    host = SD.make("AnalogData")
    x = spy.redefinetrial(_resident(host), begsample=[0, 4, 0, 0], endsample=[3, 4, 2, 5])
    assert x._data is None and np.array_equal(x.trialdefinition[:, :2], [[1, 4], [14, 14], [23, 25], [30, 35]])
    res = spy.selectdata(x, trials=[0, 1, 2], channel=[5, 0])
    assert np.array_equal(res.trialdefinition[:, :3], [[0, 3, -3], [3, 3, 0], [3, 5, -3]])
    SD.same_bits(res.data, np.concatenate([host.data[1:4], host.data[23:25]])[:, [5, 0]])
    one = spy.selectdata(_resident(host), latency=[0.0, 0.0])
    SD.same_bits(one.data, host.data[[4, 14, 26, 35]])
    cut = spy.redefinetrial(_resident(host), trials=[3, 0], toilim=[-0.2, 0.3])
    assert np.array_equal(cut.trialdefinition, [[0, 6, -2, 10], [6, 12, -2, 7]])
    SD.same_bits(cut.data, np.concatenate([host.data[33:39], host.data[2:8]]))


def test_chains_stay_on_the_device():
    """spy.selectdata(a, ...) - b, spy.copy(a) and a baseline division on resident inputs: NumPy's result, and no host
    copy of an input or an intermediate result"""
    rng = np.random.default_rng(4)
    trl = [[0, 300, -100], [300, 600, -100], [600, 900, -100]]
    xa, xb = (rng.standard_normal((900, 7)).astype(np.float32) for _ in range(2))
    a = _resident(spy.AnalogData(xa, samplerate=100.0, trialdefinition=trl))
    b = _resident(spy.AnalogData(xb[:400, :3].copy(), samplerate=100.0, trialdefinition=[[0, 200, 0], [200, 400, 0]]))
    sel = spy.selectdata(a, trials=[2, 0], channel=[6, 0, 3], latency=[0.0, 1.99])
    res = sel - b
    dup = spy.copy(a)
    assert a._data is None and b._data is None and sel._data is None and res._data is None and dup._data is None
    assert dup._device is not None and dup._device.data_ptr() != a._device.data_ptr()
    want = np.concatenate([xa[700:900], xa[100:300]])[:, [6, 0, 3]]
    SD.same_bits(res.data, want - xb[:400, :3])
    SD.same_bits(sel.data, want)
    SD.same_bits(dup.data, xa)
    assert a._data is None and b._data is None
    # float64 and a cross-spectrum stay resident too
    c = _resident(SD.make("CrossSpectralData"))
    half = spy.selectdata(c, channel_i=[1, 0], frequency=[20, 50])
    shifted = half - (1 + 1j)
    assert c._data is None and half._data is None and half._dev is not None and shifted._data is None
    with np.errstate(invalid="ignore"):
        want = SD.make("CrossSpectralData").data[:, 2:6][:, :, [1, 0]] - np.complex64(1 + 1j)
    SD.assert_identical(shifted.data, want)
    d = _resident(SD.make("SpectralData", np.float64))
    twin = spy.copy(d)
    assert d._data is None and twin._data is None and twin._resident is not None
    SD.same_bits(twin.data, SD.make("SpectralData", np.float64).data)
    assert list(twin.taper) == list(d.taper) and list(twin.freq) == list(d.freq)


def test_numpy_only_host():
    """the torch-free wrapper Device.select over the same entry point"""
    from syncopy_amd import abi
    x = SD.values((20, 2, 5, 3), np.complex64, 9)
    trials = [[12, 20], [1, 8], [5, 5], [12, 20]]
    dev = abi.Device(0)
    try:
        SD.same_bits(dev.select(x, trials), SO.gather(x, trials))
        for axes in ([None, (1, 3), None], [[1, 0, 1], None, [2, 2, 0]], [None, [4, 0], None]):
            SD.same_bits(dev.select(x, trials, axes), SO.gather(x, trials, axes))
        y = SD.values((9, 4), np.complex128, 10)
        SD.same_bits(dev.select(y, [[3, 9], [0, 2]], [[3, 3, 1]]), SO.gather(y, [[3, 9], [0, 2]], [[3, 3, 1]]))
        assert dev.select(x, [[4, 4]], [None, None, [1]]).shape == (0, 2, 5, 1)
    finally:
        dev.close()
