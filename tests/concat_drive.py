"""What the CPU emulation (tests/test_concat.py) and the GPU tests (tests/test_gpu_concat.py) of the channel concatenation
share: the emulator's driver, the route shim, the kernel cases aimed at the dispatch edges with the lane each must get,
and the front-end cases.  The kernel checks are written against a function
`join(sources, trials, pre, skew) -> (array, source addresses, output address)` that either side supplies: of trial k the
rows [trials[s][k][0], trials[s][k][1]) of every source s side by side (a row is `pre` lines), the trials stacked, as a
matrix of rows, from sources of which source s lies `skew[s]` bytes into its allocation.  Every output is filled with 0xAB
before the launch."""
import ctypes as C
import types

import numpy as np

import concat_oracle as CO
import syncopy_amd as spy
from select_drive import DT, aligned, same_bits, values  # noqa: F401  (bit for bit; the tests import them from here)
from syncopy_amd import _lib

THREADS = 256                   # of a workgroup of concat_kernel

_emu = _shim = None


def emu():
    """the library's own launcher of csrc/concat.hip on the CPU.  ctx: default launch limits; few: two workgroups"""
    global _emu
    if _emu is None:
        import build_emu
        _emu = build_emu.emulated_library("concat")
        _emu.ctx, _emu.few = build_emu.ctx(_emu), build_emu.ctx(_emu, elementwise_blocks=2)
    return _emu


def shim():
    global _shim
    if _shim is None:
        import build_emu
        _shim = build_emu.build_shim("concat_route_shim.cpp", "libconcatroute.so")
        _shim.cr_max_sources.restype = C.c_int
        _shim.cr_route.restype = C.c_int
        _shim.cr_route.argtypes = [C.c_int, C.c_int, _lib.c_i64p, _lib.c_i64p, C.c_longlong, _lib.c_i64p, C.c_longlong,
                                   C.POINTER(C.c_ulonglong), C.c_ulonglong, C.c_longlong, C.POINTER(C.c_longlong),
                                   C.POINTER(C.c_char_p)]
    return _shim


def table(trials, first=0):
    """the (ntrials, 2 + nsrc) row table of stacked trials: output row, rows, the first row in each source.
    trials: (nsrc, ntrials, 2) [start, stop) rows; a trial has the same length in every source"""
    trl = np.asarray(trials, dtype=np.int64)
    assert trl.ndim == 3 and trl.shape[2] == 2
    n = trl[0, :, 1] - trl[0, :, 0]
    assert np.array_equal(trl[:, :, 1] - trl[:, :, 0], np.broadcast_to(n, trl.shape[:2]))
    starts = first + np.concatenate(([0], np.cumsum(n)))[:-1]
    return np.ascontiguousarray(np.concatenate([starts[:, None], n[:, None], trl[:, :, 0].T], axis=1), dtype=np.int64)


def route(elem_bytes, src_rows, run, pre, desc, src_addr=None, out_addr=1 << 40, out_rows=None, nsrc=None):
    """the route's decision as a namespace (err, lane, aligned, w, row0, nrows, cum); err is the launcher's reason to
    refuse the arguments, or None"""
    nsrc = len(run) if nsrc is None else nsrc
    width = max(len(run), 1)
    desc = np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, 2 + width)
    out_rows = int(desc[:, 1].sum()) if out_rows is None else out_rows
    src_addr = [(s + 1) << 32 for s in range(width)] if src_addr is None else src_addr
    rows, runs = np.array(src_rows, dtype=np.int64), np.array(run, dtype=np.int64)
    addr = (C.c_ulonglong * max(len(src_addr), 1))(*src_addr)
    out, err = (C.c_longlong * 14)(), C.c_char_p()
    rc = shim().cr_route(elem_bytes, nsrc, rows.ctypes.data_as(_lib.c_i64p), runs.ctypes.data_as(_lib.c_i64p), pre,
                         desc.ctypes.data_as(_lib.c_i64p), desc.shape[0], addr, out_addr, out_rows, out, C.byref(err))
    if rc != 0:
        return types.SimpleNamespace(err=err.value.decode(), lane=None)
    v = list(out)
    return types.SimpleNamespace(err=None, lane=v[0], aligned=bool(v[1]), w=v[2], row0=v[3], nrows=v[4], cum=v[5:14])


def emu_concat(sources, desc, out, pre=1, ctx=None, elem_bytes=None, nsrc=None, run=None):
    """spyhip_concat of the emulated library on NumPy arrays (the arguments of backend.concat); returns its return code.
    elem_bytes, nsrc, run: what to tell the launcher instead of the arrays' own"""
    lib = emu()
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    assert all(x.flags.c_contiguous for x in sources) and out.flags.c_contiguous
    width = [int(np.prod(x.shape[1:], dtype=np.int64)) for x in sources]
    runs = np.array([w // max(pre, 1) for w in width] if run is None else run, dtype=np.int64)
    rows = np.array([x.shape[0] for x in sources], dtype=np.int64)
    ptrs = (C.c_void_p * len(sources))(*[x.ctypes.data for x in sources])
    return lib.spyhip_concat(ctx or lib.ctx, out.dtype.itemsize if elem_bytes is None else elem_bytes,
                             len(sources) if nsrc is None else nsrc, ptrs, rows.ctypes.data_as(_lib.c_i64p),
                             runs.ctypes.data_as(_lib.c_i64p), pre, desc.ctypes.data_as(_lib.c_i64p),
                             desc.ctypes.data_as(C.c_void_p), desc.shape[0], out.ctypes.data_as(C.c_void_p), out.shape[0])


def emu_join(ctx=None):
    """`join` for the kernel checks, on the emulated library"""
    def join(sources, trials, pre, skew=None):
        skew = [0] * len(sources) if skew is None else skew
        held = [aligned(x.shape, x.dtype, k) for x, k in zip(sources, skew)]
        for a, x in zip(held, sources):
            a[...] = x
        desc = table(trials)
        width = sum(int(np.prod(x.shape[1:], dtype=np.int64)) for x in sources)
        out = aligned((int(desc[:, 1].sum()), width), sources[0].dtype)
        out.view(np.uint8)[...] = 0xAB
        if out.size:
            assert emu_concat(held, desc, out, pre, ctx) == 0
        return out, [a.ctypes.data for a in held], out.ctypes.data
    return join


def emu_run(ctx=None):
    """a stand-in for concat._run that computes a plan of the front end with the emulated library"""
    def run(plan, out):
        res = np.empty((plan.nrows,) + plan.inner, dtype=plan.dtype)
        desc = np.stack([plan.starts, plan.n] + [np.array([a for a, _ in rows], dtype=np.int64) for rows in plan.rows], axis=1)
        if res.size:
            assert emu_concat([np.ascontiguousarray(o.data) for o in plan.objs], desc, res, plan.pre, ctx) == 0
        out.data = res
    return run


# ---- kernel cases ---------------------------------------------------------------------------------------------------------
def whole(sources):
    """every source whole, as one trial"""
    return [[(0, x.shape[0])] for x in sources]


def expected_lane(sources, axis, skew=None):
    """16 bytes where every run is a multiple of 16 bytes and every source begins on a 16-byte boundary, else the element"""
    eb = sources[0].dtype.itemsize
    runs = [int(np.prod(x.shape[axis:], dtype=np.int64)) for x in sources]
    fits = all(r * eb % 16 == 0 for r in runs) and not any(skew or [])
    return 16 if eb == 16 or fits else eb


def check_case(join, sources, trials, axis, lane, skew=None, what=""):
    """the joined values bit for bit, and the route's lane width for the addresses that were used"""
    shape = sources[0].shape
    pre = int(np.prod(shape[1:axis], dtype=np.int64))
    got, src_addr, out_addr = join(sources, trials, pre, skew)
    want = CO.join(sources, trials, axis)
    same_bits(got, want.reshape(want.shape[0], int(np.prod(want.shape[1:], dtype=np.int64))), what)
    run = [int(np.prod(x.shape[axis:], dtype=np.int64)) for x in sources]
    r = route(sources[0].dtype.itemsize, [x.shape[0] for x in sources], run, pre, table(trials), src_addr, out_addr)
    assert r.err is None and r.lane == lane, (what, r)
    assert lane == expected_lane(sources, axis, skew), (what, lane)
    return r


def _sources(rows, inner, chans, dtype, axis, seed=0):
    """one array per entry of `chans`: rows[s] rows of shape `inner` with chans[s] at `axis`"""
    out = []
    for s, (n, c) in enumerate(zip(rows, chans)):
        shape = (n,) + tuple(inner[:axis - 1]) + (c,) + tuple(inner[axis - 1:])
        out.append(values(shape, dtype, seed + s))
    return out


def check_element_sizes(join, name):
    """4, 8 and 16 bytes, channel fastest: runs of 4 and 8 elements are multiples of 16 bytes for every type, runs of 3 and
    4 only for complex128; two trials that begin at different rows of the two sources"""
    dtype = DT[name]
    eb = np.dtype(dtype).itemsize
    trials = [[(1, 4), (5, 10)], [(0, 3), (4, 9)]]
    check_case(join, _sources((11, 9), (), (4, 8), dtype, 1), trials, 1, 16, what=(name, "runs of 4 and 8"))
    check_case(join, _sources((11, 9), (), (3, 4), dtype, 1, 2), trials, 1, 16 if eb == 16 else eb, what=(name, "runs of 3 and 4"))
    check_case(join, _sources((11, 9), (2, 3), (4, 2), dtype, 3, 4), trials, 3, 16 if eb >= 8 else eb, what=(name, "pre = 6"))
    check_case(join, _sources((11, 9), (6,), (1, 2), dtype, 1, 6), trials, 1, 16 if eb >= 8 else eb, what=(name, "channel in the middle"))


def check_lanes(join):
    """float32 around the 16-byte boundary, and a complex128 source on an 8-byte boundary"""
    trials = [[(0, 5), (5, 7)], [(2, 7), (0, 2)]]
    a = _sources((7, 7), (), (4, 8), np.float32, 1)
    assert check_case(join, a, trials, 1, 16, what="runs (4, 8), aligned").aligned
    check_case(join, _sources((7, 7), (), (3, 4), np.float32, 1, 2), trials, 1, 4, what="runs (3, 4)")
    check_case(join, _sources((7, 7), (), (4, 6), np.float32, 1, 2), trials, 1, 4, what="runs (4, 6): 24 bytes")
    for skew in ([4, 0], [0, 4], [8, 0], [0, 8], [12, 12]):
        check_case(join, a, trials, 1, 4, skew=skew, what=("runs (4, 8), a source off the boundary", skew))
    d = _sources((7, 7), (), (2, 4), np.float64, 1, 4)
    check_case(join, d, trials, 1, 16, what="float64, runs (2, 4)")
    check_case(join, d, trials, 1, 8, skew=[0, 8], what="float64, runs (2, 4), a source 8 bytes off")
    z = _sources((7, 7), (), (3, 2), np.complex128, 1, 6)
    assert check_case(join, z, trials, 1, 16, what="complex128").aligned
    for skew in ([8, 0], [0, 8], [8, 8]):
        r = check_case(join, z, trials, 1, 16, skew=skew, what=("complex128, a source 8 bytes off", skew))
        assert not r.aligned


def check_layouts(join):
    """pre = 1 and pre = 6 with channel fastest, and channel in the middle (run = channels x 6), each with runs that get
    16-byte lanes and runs that get element lanes"""
    trials = [[(3, 6), (0, 3), (6, 10)], [(0, 3), (3, 6), (6, 10)]]
    for chans, lane in (((4, 8), 16), ((1, 3), 4), ((5, 2), 4)):
        check_case(join, _sources((10, 10), (), chans, np.float32, 1), trials, 1, lane, what=("pre = 1", chans))
        check_case(join, _sources((10, 10), (2, 3), chans, np.float32, 3, 2), trials, 3, lane, what=("pre = 6", chans))
    for chans, lane in (((2, 4), 16), ((1, 3), 4), ((2, 1), 4)):    # runs of 6 x channels: 24-byte units
        check_case(join, _sources((10, 10), (6,), chans, np.float32, 1, 4), trials, 1, lane, what=("channel in the middle", chans))
        check_case(join, _sources((10, 10), (3, 2), chans, np.float32, 1, 6), trials, 1, lane, what=("channel, taper, freq", chans))
    check_case(join, _sources((10, 10), (5, 3), (2, 1), np.complex64, 2, 8), trials, 2, 8, what="channel between two axes")
    check_case(join, _sources((10, 10), (5, 2), (2, 1), np.complex64, 2, 8), trials, 2, 16, what="channel between two axes, 16-byte runs")


def check_sources(join):
    """2, 3 and 8 sources with unequal runs, a run of 1 included; the same source twice"""
    for chans, lane in (((1, 5), 4), ((5, 1), 4), ((3, 1, 4), 4), ((1, 2, 3, 4, 5, 6, 7, 8), 4), ((4, 8, 4), 16),
                        ((4, 8, 4, 12, 4, 4, 8, 16), 16), ((1, 1, 1, 1, 1, 1, 1, 1), 4)):
        rows = tuple(9 + s for s in range(len(chans)))
        trials = [[(s % 3, 4 + s % 3), (4 + s % 2, 8 + s % 2)] for s in range(len(chans))]
        src = _sources(rows, (), chans, np.float32, 1, len(chans))
        check_case(join, src, trials, 1, lane, what=("channel fastest", chans))
        src = _sources(rows, (2,), chans, np.float32, 2, len(chans))
        check_case(join, src, trials, 2, lane, what=("pre = 2", chans))
    one = values((6, 4), np.float32, 30)
    check_case(join, [one, one, one], [[(0, 3)], [(3, 6)], [(0, 3)]], 1, 16, what="one source three times")


def check_trials(join):
    """the trial table: sources whose trials begin at different rows, a repeat, a reversal, trials of 0 rows, one trial"""
    src = _sources((12, 14), (2,), (4, 8), np.float32, 2, 40) + _sources((12,), (2,), (3,), np.float32, 2, 42)
    three = [(0, 4), (4, 9), (9, 12)]
    other = [(2, 6), (7, 12), (0, 3)]                                         # the same lengths, elsewhere
    for what, a, b in (("one trial", [(2, 7)], [(9, 14)]),
                       ("a repeat and a reversal", [three[k] for k in (2, 0, 0, 1)], [other[k] for k in (2, 0, 0, 1)]),
                       ("overlapping source trials", [(0, 6), (3, 9), (2, 12)], [(1, 7), (0, 6), (4, 14)]),
                       ("a trial of 0 rows between two others", [(0, 3), (5, 5), (2, 4)], [(11, 14), (0, 0), (3, 5)]),
                       ("trials of 0 rows first and last", [(1, 1), (0, 3), (12, 12)], [(14, 14), (5, 8), (0, 0)]),
                       ("trials of 0 rows only", [(1, 1), (4, 4)], [(0, 0), (14, 14)]), ("one row", [(7, 8)], [(13, 14)])):
        check_case(join, src[:2], [a, b], 2, 16, what=what)
        check_case(join, [src[0], src[2], src[1]], [a, a, b], 2, 4, what=what)


def check_few_workgroups(join, blocks=2):
    """more lanes than `blocks` workgroups cover in one round, so that every workgroup walks several: an output that ends
    exactly on a workgroup boundary and one lane to either side of it, in element lanes and in 16-byte lanes; and several
    trials of several rows"""
    edge = 3 * blocks * THREADS                                  # lanes: three full rounds
    for lanes in (edge - 1, edge, edge + 1, edge - THREADS, edge - THREADS + 1):
        left = lanes // 2 - 67
        src = _sources((2, 3), (), (left, lanes - left), np.float32, 1, lanes)
        check_case(join, src, [[(1, 2)], [(2, 3)]], 1, 4, what=("element lanes", lanes))
        wide = _sources((2, 3), (), (4 * left, 4 * (lanes - left)), np.float32, 1, lanes)
        check_case(join, wide, [[(1, 2)], [(2, 3)]], 1, 16, what=("16-byte lanes", lanes))
    src = _sources((40, 45), (3,), (5, 6), np.float32, 2, 50)   # 37 rows of 33 elements
    check_case(join, src, [[(0, 17), (20, 40)], [(25, 42), (0, 20)]], 2, 4, what="several trials, element lanes")
    src = _sources((40, 45), (3,), (4, 8), np.complex64, 2, 52)
    check_case(join, src, [[(0, 17), (20, 40)], [(25, 42), (0, 20)]], 2, 16, what="several trials, 16-byte lanes")


# ---- front-end cases ---------------------------------------------------------------------------------------------------------
MIDDLE = ["time", "channel", "taper", "freq"]


def make(cls, nchan=6, dtype=None, seed=0, prefix="ch", shift=0, dimord=None):
    """an object with `nchan` labelled channels, unequal trials that begin `shift` (0, 1 or 2) rows later than those of
    shift 0 in a recording of the same length, gaps between them and (AnalogData, TimeLockData) an extra trial column"""
    names = [f"{prefix}{i}" for i in range(nchan)]
    if cls in ("AnalogData", "TimeLockData"):
        trl = np.array([[1, 10, -3, 7], [10, 22, -4, 8], [23, 30, -3, 9], [30, 41, -5, 10]], dtype=float)
        trl[:, :2] += shift
        x = values((43, nchan), dtype or np.float32, seed)
        return getattr(spy, cls)(x, samplerate=10.0, trialdefinition=trl, channel=names)
    assert cls == "SpectralData"
    trl = np.array([[0, 5, -2], [5, 9, -1], [9, 14, -2]], dtype=float)
    trl[:, :2] += shift
    shape = (16, nchan, 2, 3) if dimord == MIDDLE else (16, 2, 3, nchan)
    s = spy.SpectralData(values(shape, dtype or np.complex64, seed), samplerate=10.0, trialdefinition=trl, dimord=dimord)
    s.freq, s.taper, s.channel = np.arange(3) * 10.0, np.array(["t0", "t1"]), np.array(names)
    return s


# class, dimord of the objects of the end-to-end cases
FRONT_CASES = [("AnalogData", None), ("SpectralData", None), ("SpectralData", MIDDLE), ("TimeLockData", None)]


def make_pair(case, dtype=None):
    """two objects of FRONT_CASES[case] with 6 and 4 channels, distinct labels and trials at different rows"""
    cls, dimord = FRONT_CASES[case]
    return [make(cls, 6, dtype, 1, "a", 0, dimord), make(cls, 4, dtype, 2, "b", 2, dimord)]


def check_frontend(objs, hosts):
    """spy.concat(*objs) against the oracle on `hosts` (the same objects with their data on the host): the data bit for
    bit, the trialdefinition, the labels, the cfg"""
    res = spy.concat(*objs)
    data, trl, labels = CO.concat(hosts)
    first = objs[0]
    assert type(res) is type(first) and res.dimord == first.dimord and res.samplerate == first.samplerate
    same_bits(res.data, data)
    assert np.array_equal(res.trialdefinition, trl), (res.trialdefinition, trl)
    if labels == "default":
        if isinstance(res, spy.AnalogData):
            assert list(res.channel) == list(spy.AnalogData(np.zeros((1, data.shape[-1]), dtype=np.float32), samplerate=1.0).channel)
        else:
            assert res.channel is None
    else:
        assert list(res.channel) == labels
    for prop in ("freq", "taper"):
        if getattr(first, prop, None) is not None:
            assert list(getattr(res, prop)) == list(getattr(first, prop))
    assert res.cfg["concat"] == {"dim": "channel", "objects": len(objs), "channels": [len(h.channel) for h in hosts]}
    assert res.selection is None
    if isinstance(res, spy.TimeLockData):
        assert res.avg is None and res.var is None and res.cov is None
    return res
