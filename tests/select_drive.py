"""What the CPU emulation (tests/test_select.py) and the GPU tests (tests/test_gpu_select.py) of the data selection share:
the emulator's driver, the route shim, the kernel cases aimed at the dispatch edges with the lane each must get, and the
front-end cases of the four data classes.  The kernel checks are written against a function
`gather(src, trials, axes, skew) -> (array, source address, output address)` that either side supplies: the trials'
[start, stop) rows of `src`, of every row what `axes` names, from a source that lies `skew` bytes into its allocation."""
import ctypes as C
import types

import numpy as np

import select_oracle as SO
import syncopy_amd as spy
from arith_drive import assert_identical  # noqa: F401  (bit for bit; the tests import it from here)
from syncopy_amd import _lib
from syncopy_amd.datatype.selectdata import select_axes

FLAT, AXES, AXES_LDS = 0, 1, 2
DT = {"f4": np.float32, "f8": np.float64, "c8": np.complex64, "c16": np.complex128}

_emu = _shim = None


def emu():
    """the library's own launcher of csrc/select.hip on the CPU.  ctx: default launch limits; few: two workgroups"""
    global _emu
    if _emu is None:
        import build_emu
        _emu = build_emu.emulated_library("select")
        _emu.ctx, _emu.few = build_emu.ctx(_emu), build_emu.ctx(_emu, elementwise_blocks=2)
    return _emu


def shim():
    global _shim
    if _shim is None:
        import build_emu
        _shim = build_emu.build_shim("select_route_shim.cpp", "libselectroute.so")
        _shim.sr_lds_cap.restype = C.c_longlong
        _shim.sr_route.restype = C.c_int
        _shim.sr_route.argtypes = [C.c_int, C.c_longlong, C.c_longlong, _lib.c_i64p, _lib.c_i32p, _lib.c_i64p, _lib.c_i64p,
                                   _lib.c_i32p, _lib.c_i64p, C.c_longlong, C.c_ulonglong, C.c_ulonglong,
                                   C.POINTER(C.c_longlong)]
    return _shim


def lds_cap():
    return int(shim().sr_lds_cap())


def table(trials, first=0):
    """the (ntrials, 3) row table of stacked trials: output row, source row, rows"""
    trl = np.asarray(trials, dtype=np.int64).reshape(-1, 2)
    n = trl[:, 1] - trl[:, 0]
    starts = first + np.concatenate(([0], np.cumsum(n)))[:-1]
    return np.ascontiguousarray(np.stack([starts, trl[:, 0], n], axis=1), dtype=np.int64)


def _axis_args(inner, axes):
    extent, kind, start, count, idx = select_axes(inner, axes)
    p64 = lambda x: x.ctypes.data_as(_lib.c_i64p)                                       # noqa: E731
    return (p64(extent), kind.ctypes.data_as(_lib.c_i32p), p64(start), p64(count),
            None if idx is None else idx.ctypes.data_as(_lib.c_i32p)), (extent, kind, start, count, idx)


def route(elem_bytes, src_rows, inner, trials, axes, src_addr=0, out_addr=1 << 40, out_rows=None, desc=None):
    """the route's decision as a namespace (mode, lane, aligned, run, wo, ws, n, s, start, loff, nidx), or None where the
    launcher refuses the arguments"""
    desc = table(trials) if desc is None else np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, 3)
    out_rows = int(desc[:, 2].sum()) if out_rows is None else out_rows
    args, keep = _axis_args(inner, axes)
    out = (C.c_longlong * 19)()
    rc = shim().sr_route(elem_bytes, src_rows, out_rows, *args, desc.ctypes.data_as(_lib.c_i64p), desc.shape[0], src_addr,
                         out_addr, out)
    if rc != 0:
        return None
    v = list(out)
    return types.SimpleNamespace(mode=v[0], lane=v[1], aligned=bool(v[2]), run=v[3], wo=v[4], ws=v[5], n=v[6:9], s=v[9:12],
                                 start=v[12:15], loff=v[15:18], nidx=v[18])


def emu_select(src, desc, out, axes=None, ctx=None):
    """spyhip_select of the emulated library on NumPy arrays (the arguments of backend.select); returns its return code"""
    lib = emu()
    desc = np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, 3)
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype
    args, keep = _axis_args(src.shape[1:], axes)
    idx = keep[4]
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)                # noqa: E731
    return lib.spyhip_select(ctx or lib.ctx, src.dtype.itemsize, ptr(src), src.shape[0], *args, ptr(idx),
                             desc.ctypes.data_as(_lib.c_i64p), ptr(desc), desc.shape[0], ptr(out), out.shape[0])


def aligned(shape, dtype, skew=0):
    """an uninitialised C-contiguous array that begins `skew` bytes behind a 16-byte boundary"""
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    raw = np.empty(nbytes + 32, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16 + skew
    return raw[at:at + nbytes].view(dtype).reshape(shape)


def emu_gather(ctx=None):
    """`gather` for the kernel checks, on the emulated library"""
    def gather(src, trials, axes, skew=0):
        a = aligned(src.shape, src.dtype, skew)
        a[...] = src
        desc = table(trials)
        count = select_axes(src.shape[1:], axes)[3]
        out = aligned((int(desc[:, 2].sum()),) + tuple(int(c) for c in count[4 - src.ndim:]), src.dtype)
        out.view(np.uint8)[...] = 0xAB
        if out.size:
            assert emu_select(a, desc, out, axes, ctx) == 0
        return out, a.ctypes.data, out.ctypes.data
    return gather


def emu_run(ctx=None):
    """a stand-in for selectdata._run that computes a plan of the front end with the emulated library"""
    def run(plan, out):
        res = np.empty((plan.nrows,) + plan.inner, dtype=plan.dtype)
        n = [b - a for a, b in plan.rows]
        desc = np.stack([plan.starts, [a for a, _ in plan.rows], n], axis=1)
        if res.size:
            assert emu_select(np.ascontiguousarray(plan.base.data), desc, res, plan.axes, ctx) == 0
        out.data = res
    return run


# ---- kernel cases ---------------------------------------------------------------------------------------------------------
def values(shape, dtype, seed=0):
    """random bits of `dtype`, with NaN payloads, signed zeros and infinities among them"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    x = x.astype(dtype)
    flat = x.reshape(-1).view(np.float32 if x.real.dtype == np.float32 else np.float64)
    flat[::7] = -0.0
    flat[3::11] = np.inf
    bits = flat.view(np.uint32 if flat.dtype == np.float32 else np.uint64)
    bits[5::13] = bits.dtype.type(0x7FC01234 if flat.dtype == np.float32 else 0x7FF8000000ABCDEF)   # quiet NaNs with a payload
    bits[6::17] = bits.dtype.type(0xFFC00001 if flat.dtype == np.float32 else 0xFFF8000000000001)
    return x


def same_bits(got, want, what=""):
    """same dtype, shape and bytes: NaN payloads and the signs of zeros included"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert np.array_equal(g, w), (what, int((g != w).sum()))


def check_case(gather, src, trials, axes, lane, mode=None, skew=0, what=""):
    """the gathered values bit for bit, and the route's lane width (and mode) for the addresses that were used"""
    got, src_addr, out_addr = gather(src, trials, axes, skew)
    same_bits(got, SO.gather(src, trials, axes), what)
    r = route(src.dtype.itemsize, src.shape[0], src.shape[1:], trials, axes, src_addr, out_addr)
    assert r is not None and r.lane == lane, (what, r)
    assert mode is None or r.mode == mode, (what, r)
    return r


def check_element_sizes(gather, name):
    """4, 8 and 16 bytes through the whole-row, range, fastest-axis-list and middle-axis-list routes.  Rows of 3 x 5 x 8
    elements: every row, every run of 4 or 8 channels and every middle-axis step is a multiple of 16 bytes, so all but
    the fastest-axis list move 16 bytes per lane"""
    dtype = DT[name]
    eb = np.dtype(dtype).itemsize
    src = values((11, 3, 5, 8), dtype)
    trials = [(1, 4), (6, 11)]
    check_case(gather, src, trials, None, 16, FLAT, what=(name, "whole rows"))
    check_case(gather, src, trials, [None, None, (4, 4)], 16, AXES, what=(name, "range"))
    check_case(gather, src, trials, [None, None, [7, 0, 0, 3]], eb, AXES_LDS, what=(name, "fastest-axis list"))
    check_case(gather, src, trials, [None, [4, 1, 1], None], 16, AXES_LDS, what=(name, "middle-axis list"))
    check_case(gather, src, trials, [[2, 0], (1, 3), [5]], eb, AXES_LDS, what=(name, "list, range, list"))
    check_case(gather, src, trials, [(1, 2), None, None], 16, AXES, what=(name, "range over whole axes"))


def check_boundary(gather):
    """float32 around the 16-byte boundary: 16-byte lanes need runs of a multiple of 4 elements that begin on a multiple
    of 4 elements in both tensors"""
    src8, src7 = values((9, 8), np.float32, 1), values((9, 7), np.float32, 2)
    trials = [(1, 4), (5, 9)]
    for count in (3, 4, 5, 8):
        for start in (0, 1, 2, 3):
            if start + count > 8:
                continue
            lane = 16 if count % 4 == 0 and start % 4 == 0 else 4
            r = check_case(gather, src8, trials, [(start, count)], lane, what=("range", start, count))
            assert r.run == (8 if count == 8 else count) and r.mode == (FLAT if count == 8 else AXES)
    # 7 channels: every second row starts off the boundary
    check_case(gather, src7, trials, [(0, 4)], 4, AXES, what="7 channels, rows of a trial off the boundary")
    check_case(gather, src7, [(4, 5)], [(0, 4)], 16, AXES, what="7 channels, one row that starts on the boundary")
    check_case(gather, src7, [(1, 2)], [(0, 4)], 4, AXES, what="7 channels, one row that starts off it")
    check_case(gather, src7, [(0, 4), (4, 8)], None, 16, FLAT, what="7 channels, whole trials of 28 elements")
    check_case(gather, src7, [(1, 5)], None, 4, FLAT, what="7 channels, a trial that starts at element 7")
    check_case(gather, src7, [(0, 3), (4, 8)], None, 4, FLAT, what="7 channels, a trial of 21 elements")
    # a source that is a view starting 4 bytes into its allocation
    check_case(gather, src8, trials, None, 4, FLAT, skew=4, what="whole rows of a source 4 bytes off")
    check_case(gather, src8, trials, [(4, 4)], 4, AXES, skew=4, what="range of a source 4 bytes off")
    # the 8-byte types have a boundary of 2 elements
    z = values((6, 5), np.complex64, 3)
    check_case(gather, z, [(0, 6)], [(2, 2)], 8, AXES, what="complex64, rows of 5 elements")
    check_case(gather, z, [(2, 3)], [(2, 2)], 16, AXES, what="complex64, one row at element 10, start 2")
    check_case(gather, z, [(0, 2), (2, 6)], None, 16, FLAT, what="complex64, whole trials")


def check_trials(gather):
    """rows of 2 x 4 float32: whole trials always move 16 bytes per lane, a list on the fastest axis never"""
    src = values((12, 2, 4), np.float32, 4)
    three = [(0, 4), (4, 9), (9, 12)]
    for what, trials in (("one trial", [(2, 7)]), ("a repeat and a reversal", [three[k] for k in (2, 0, 0, 1)]),
                         ("overlapping source trials", [(0, 6), (3, 9), (2, 12)]),
                         ("a trial of 0 rows between two others", [(0, 3), (5, 5), (2, 4)]),
                         ("trials of 0 rows first and last", [(1, 1), (0, 3), (12, 12)]), ("one row", [(7, 8)])):
        check_case(gather, src, trials, None, 16, FLAT, what=what)
        check_case(gather, src, trials, [None, [2, 0, 3]], 4, AXES_LDS, what=what)


def check_index_lists(gather):
    """length 1, unsorted with repeats, and the LDS cap: a middle axis of `cap` and `cap + 1` entries (over 5 frequencies)
    in front of two channels"""
    cap = lds_cap()
    src = values((3, 1, 5, 2), np.float32, 5)
    trials = [(0, 2), (2, 3)]
    rng = np.random.default_rng(6)
    check_case(gather, src, trials, [None, [3], None], 4, AXES_LDS, what="one entry")
    check_case(gather, src, trials, [None, [4, 0, 4, 2, 2, 1], [1, 1, 0]], 4, AXES_LDS, what="unsorted with repeats")
    r = check_case(gather, src, trials, [None, rng.integers(0, 5, cap), None], 4, AXES_LDS, what="the cap")
    assert r.nidx == cap and r.n == [1, cap, 2]
    r = check_case(gather, src, trials, [None, rng.integers(0, 5, cap + 1), None], 4, AXES, what="the cap and one")
    assert r.nidx == cap + 1
    # lists that repeat the one entry of an axis of extent 1, slow, middle and fastest; at the cap and beyond it
    one = values((3, 1, 5), np.float32, 8)
    r = check_case(gather, one, trials, [[0, 0, 0], None], 4, AXES_LDS, what="a repeated list on a slow axis of extent 1")
    assert (r.wo, r.ws, r.n, r.s) == (15, 5, [1, 3, 5], [0, 5, 1])
    check_case(gather, values((3, 4, 1, 4), np.float32, 9), trials, [None, [0, 0], None], 16, AXES_LDS,
               what="a repeated list on a middle axis of extent 1")
    r = check_case(gather, values((3, 4, 1), np.float32, 10), trials, [None, [0, 0, 0]], 4, AXES_LDS,
                   what="a repeated list on a fastest axis of extent 1")
    assert (r.wo, r.ws, r.n) == (12, 4, [1, 4, 3])
    check_case(gather, values((3, 1, 2), np.float32, 11), trials, [np.zeros(cap, dtype=np.int32), None], 4, AXES_LDS,
               what="the cap on an axis of extent 1")
    check_case(gather, values((3, 1, 2), np.float32, 11), trials, [np.zeros(cap + 1, dtype=np.int32), None], 4, AXES,
               what="the cap and one on an axis of extent 1")
    wide = values((2, 1, 5, 4), np.float32, 7)                               # runs of 4 channels: 16-byte lanes, list in LDS
    check_case(gather, wide, [(0, 2)], [None, [4, 4, 0], None], 16, AXES_LDS, what="a list in front of 16-byte runs")


# ---- front-end cases ---------------------------------------------------------------------------------------------------------
def make(cls, dtype=None, seed=0):
    """an object of one of the four classes with labels, unequal trials, gaps between them and an extra trial column"""
    if cls in ("AnalogData", "TimeLockData"):
        trl = [[1, 10, -3, 7], [10, 22, -4, 8], [23, 30, -3, 9], [30, 41, -5, 10]]
        x = values((43, 6), dtype or np.float32, seed)
        names = [f"ch{i}" for i in range(6)]
        if cls == "AnalogData":
            return spy.AnalogData(x, samplerate=10.0, trialdefinition=trl, channel=names)
        return spy.TimeLockData(x, samplerate=10.0, trialdefinition=trl, channel=names)
    if cls in ("SpectralData", "SpectralData, one taper"):
        ntaper = 4 if cls == "SpectralData" else 1
        s = spy.SpectralData(values((14, ntaper, 9, 5), dtype or np.complex64, seed), samplerate=10.0,
                             trialdefinition=[[0, 5, -2], [5, 9, -1], [9, 14, -2]])
        s.freq, s.taper = np.arange(9) * 10.0, np.array([f"t{i}" for i in range(ntaper)])
        s.channel = np.array([f"ch{i}" for i in range(5)])
        return s
    c = spy.CrossSpectralData(values((6, 9, 4, 4), dtype or np.complex64, seed), samplerate=10.0,
                              trialdefinition=[[0, 2, 0], [2, 4, 0], [4, 6, 0]])
    c.freq = np.arange(9) * 10.0
    c.channel_i, c.channel_j = np.array([f"a{i}" for i in range(4)]), np.array([f"b{i}" for i in range(4)])
    return c


# the selections of the issue, class by class; trial 2 of the AnalogData / TimeLockData object does not cover the window
FRONT_CASES = [
    ("AnalogData", {"trials": [3, 1, 2, 1], "channel": ["ch4", "ch0", "ch1"], "latency": [-0.3, 0.4]}),
    ("AnalogData", {"trials": [2, 0]}),
    ("AnalogData", {"channel": slice(2, 6)}),
    ("SpectralData", {"taper": [3, 0], "frequency": [30, 60], "channel": ["ch3", "ch1", "ch2"]}),
    ("SpectralData", {"trials": [2, 2, 0], "latency": [-0.1, 0.1], "taper": "t1"}),
    ("CrossSpectralData", {"channel_i": [3, 0, 0], "channel_j": slice(1, 3), "frequency": 42.0}),
    ("CrossSpectralData", {"trials": [1], "frequency": [0, 80]}),
    ("TimeLockData", {"trials": [0, 3], "channel": range(1, 4), "latency": [-0.2, 0.2]}),
    # a list that repeats the one entry of an axis of extent 1: the axis grows
    ("SpectralData, one taper", {"taper": [0, 0]}),
    ("SpectralData, one taper", {"trials": [2, 0], "taper": ["t0", "t0", "t0"], "frequency": [30, 60], "channel": [4, 4]}),
]


def check_frontend(obj, host, kwargs):
    """spy.selectdata(obj, **kwargs) against the oracle on `host` (the same object with its data on the host): the data
    bit for bit, the trialdefinition, the labels, the cfg; and nothing of `obj` touched"""
    before = None if obj.selection is None else dict(obj.selection.select)
    res = spy.selectdata(obj, **kwargs)
    data, trl, labels = SO.selectdata(host, **kwargs)
    assert type(res) is type(obj) and res.dimord == obj.dimord and res.samplerate == obj.samplerate
    same_bits(res.data, data, kwargs)
    assert np.array_equal(res.trialdefinition, trl), (res.trialdefinition, trl)
    for dim, want in labels.items():
        got = getattr(res, dim, None)
        assert (got is None and want is None) or list(got) == list(want), (dim, got, want)
    assert set(kwargs) <= set(res.cfg["selectdata"]) and res.cfg["selectdata"]["inplace"] is False
    assert res.selection is None
    assert (None if obj.selection is None else dict(obj.selection.select)) == before
    if isinstance(res, spy.TimeLockData):
        assert res.avg is None and res.var is None and res.cov is None
    return res
