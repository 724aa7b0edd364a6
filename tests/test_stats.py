"""spy.var / spy.std / spy.median / spy.itc without a GPU: the front end driven by the NumPy model (stats_oracle.py), its
argument checks, and a CPU emulation of the kernels of syncopy_amd/csrc/stats_kernel.h against NumPy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import syncopy_amd as spy
import stats_oracle as SO
from parity import assert_parity
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "mean_variants.npz"))
HOW = dict(compute_method="sequential", routine_classes=SO.STATS_OPS)


def _analog():
    return spy.AnalogData(np.concatenate(list(Z["data"])), samplerate=float(Z["samplerate"]),
                          trialdefinition=Z["trialdefinition"])


def _spectral(key="spec"):
    s = spy.SpectralData(Z[key], samplerate=float(Z["samplerate"]), trialdefinition=Z["spec_trldef"])
    s.channel = np.array(["channel%d" % (i + 1) for i in range(Z[key].shape[-1])])
    s.freq = np.arange(Z[key].shape[2], dtype=float)
    return s


def _trials(data):
    return [np.asarray(t) for t in data.trials]


# ---- the front end with the oracle ops --------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["var", "std"])
@pytest.mark.parametrize("src", ["analog", "spec", "pow"])
def test_trial_var_std_front_end(op, src):
    data = _analog() if src == "analog" else _spectral(src)
    out = getattr(spy, op)(data, dim="trials", **HOW)
    ref = getattr(SO, "trial_" + op)(_trials(data))
    assert out.data.dtype == data.data.dtype and out.data.shape == ref.shape
    assert np.array_equal(out.data, ref)
    assert np.asarray(out.trialdefinition).shape == (1, 3)
    assert np.asarray(out.trialdefinition)[0, 1] - np.asarray(out.trialdefinition)[0, 0] == ref.shape[0]
    if np.iscomplexobj(out.data):
        assert np.all(out.data.imag == 0)


@pytest.mark.parametrize("op", ["var", "std", "median"])
def test_axis_ops_shapes_labels_and_trialdefinition(op):
    fn = getattr(spy, op)
    out = fn(_analog(), dim="time", **HOW)
    assert out.data.shape == (6, 5) and out.data.dtype == np.float32
    assert np.array_equal(np.asarray(out.trialdefinition, float)[:, :2], np.c_[np.arange(6), np.arange(1, 7)])
    ref = np.concatenate([getattr(SO, "axis_" + op)(x, 0) for x in Z["data"]])
    assert np.array_equal(out.data, ref, equal_nan=True)

    out = fn(_analog(), dim="channel", **HOW)
    assert out.data.shape == (1800, 1) and list(out.channel) == [op]
    assert np.array_equal(np.asarray(out.trialdefinition, float), Z["trialdefinition"].astype(float))

    spec = _spectral()
    out = fn(spec, dim="freq", **HOW)
    assert out.data.shape == (6, 5, 1, 5) and out.data.dtype == np.complex64 and out.freq is None
    assert list(out.channel) == list(spec.channel)
    if op != "median":
        assert np.all(out.data.imag == 0)

    out = fn(spec, dim="channel", keeptrials=False, **HOW)
    assert out.data.shape == (1, 5, 151, 1) and list(out.channel) == [op]
    assert np.array_equal(out.freq, spec.freq)
    per = [getattr(SO, "axis_" + op)(x, 3) for x in _trials(spec)]
    assert np.array_equal(out.data, SO.trial_mean(per))

    out = fn(_analog(), dim="time", keeptrials=False, **HOW)
    assert out.data.shape == (1, 5)
    assert np.array_equal(np.asarray(out.trialdefinition, float), [[0, 1, 0]])


def test_axis_ops_with_selection():
    sel = {"trials": [0, 2, 3], "channel": [0, 3]}
    data = _analog()
    out = spy.var(data, dim="time", select=sel, **HOW)
    trials = [np.ascontiguousarray(x[:, [0, 3]]) for x in _trials(data)]    # (fancy indexing alone gives F order)
    ref = np.concatenate([SO.axis_var(trials[t], 0) for t in (0, 2, 3)])
    assert np.array_equal(out.data, ref)
    assert list(out.channel) == [data.channel[0], data.channel[3]]
    assert data.selection is None
    out = spy.std(data, dim="trials", select=sel, **HOW)
    assert np.array_equal(out.data, SO.trial_std([trials[t] for t in (0, 2, 3)]))


def test_itc_front_end():
    spec = _spectral()
    out = spy.itc(spec, **HOW)
    ref = SO.itc(_trials(spec), 1)
    assert out.data.dtype == np.float32 and out.data.shape == (1, 1, 151, 5)
    assert np.array_equal(out.data, ref, equal_nan=True)
    assert out.taper is None and np.array_equal(out.freq, spec.freq) and list(out.channel) == list(spec.channel)
    assert np.nanmax(out.data) <= 1 + 1e-6 and np.nanmin(out.data) >= 0
    out = spy.itc(spec, select={"trials": [1, 4]}, **HOW)
    assert np.array_equal(out.data, SO.itc([_trials(spec)[1], _trials(spec)[4]], 1), equal_nan=True)


def test_argument_errors():
    with pytest.raises(SPYValueError, match="output='fourier"):
        spy.itc(_spectral("pow"), **HOW)
    with pytest.raises(SPYTypeError):
        spy.itc(_analog(), **HOW)
    with pytest.raises(NotImplementedError, match="Trial median"):
        spy.median(_analog(), dim="trials", **HOW)
    uneq = spy.AnalogData(np.zeros((30, 2), np.float32), samplerate=10.0,
                          trialdefinition=np.array([[0, 10, 0], [10, 30, 0]]))
    for fn in (spy.var, spy.std):
        with pytest.raises(SPYValueError):
            fn(uneq, dim="trials", **HOW)
    with pytest.raises(SPYValueError):
        spy.var(_analog(), dim="freq", **HOW)
    with pytest.raises(SPYValueError):
        spy.median(_analog(), dim="nonsense", **HOW)
    f64 = spy.AnalogData(np.zeros((30, 2)), samplerate=10.0, trialdefinition=np.array([[0, 15, 0], [15, 30, 0]]))
    for fn in (spy.var, spy.std, spy.median):
        with pytest.raises(SPYTypeError):
            fn(f64, dim="time")                 # the device route takes float32 / complex64 only
    c128 = spy.SpectralData(Z["spec"].astype(np.complex128), samplerate=1.0, trialdefinition=Z["spec_trldef"])
    with pytest.raises(SPYTypeError):
        spy.itc(c128)


# ---- CPU emulation of stats_kernel.h ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(HERE, "emu", "stats_emu.cpp")
    out = os.path.join(HERE, "emu", "_build", "libstatsemu.so")
    csrc = os.path.join(HERE, "..", "syncopy_amd", "csrc")
    deps = [src, os.path.join(HERE, "emu", "hip_emu.h"), os.path.join(csrc, "stats_kernel.h"), os.path.join(csrc, "np_sum.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        cxx = clang if os.path.exists(clang) else "g++"
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-x", "c++", src, "-o", out])
    lib = C.CDLL(out)
    ll, vp = C.c_longlong, C.c_void_p
    lib.emu_trial_var.argtypes = [vp, vp, vp, vp, ll, ll, C.c_int, C.c_int, ll]
    lib.emu_itc.argtypes = [vp, vp, vp, ll, ll, ll, ll, ll]
    lib.emu_axis_nanvar.argtypes = [vp, ll, ll, ll, C.c_int, C.c_int, vp]
    lib.emu_axis_nanmedian.argtypes = [vp, ll, ll, ll, C.c_int, vp, vp, C.c_uint]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _split(shape, axis):
    return int(np.prod(shape[:axis])), shape[axis], int(np.prod(shape[axis + 1:]))


def emu_trial_var(lib, x, take_sqrt, chunk=None):
    x = np.ascontiguousarray(x)
    T, shape = x.shape[0], x.shape[1:]
    cplx = np.iscomplexobj(x)
    mean = np.zeros(shape, x.dtype)
    acc = np.zeros(shape, np.float32)
    out = np.empty(shape, x.dtype)
    lib.emu_trial_var(_p(x), _p(mean), _p(acc), _p(out), T, int(np.prod(shape)), int(cplx), int(take_sqrt), chunk or T)
    return out


def emu_itc(lib, x, taper_axis, chunk=None):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    T, shape = x.shape[0], x.shape[1:]
    outer, K, inner = _split(shape, taper_axis)
    acc = np.zeros(shape, np.complex64)
    oshape = list(shape)
    oshape[taper_axis] = 1
    out = np.empty(oshape, np.float32)
    lib.emu_itc(_p(x), _p(acc), _p(out), T, outer, K, inner, chunk or T)
    return out


def emu_axis(lib, x, axis, op, nblocks=3):
    x = np.ascontiguousarray(x)
    outer, n, inner = _split(x.shape, axis)
    oshape = list(x.shape)
    oshape[axis] = 1
    out = np.empty(oshape, x.dtype)
    cplx = int(np.iscomplexobj(x))
    if op == "median":
        work = np.empty_like(x)
        lib.emu_axis_nanmedian(_p(x), outer, n, inner, cplx, _p(work), _p(out), nblocks)
    else:
        lib.emu_axis_nanvar(_p(x), outer, n, inner, cplx, int(op == "std"), _p(out))
    return out


def _edge(rng, shape, cplx):
    x = rng.normal(size=shape).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.normal(size=shape)).astype(np.complex64)
    flat = x.reshape(-1)
    k = flat.size
    idx = rng.permutation(k)
    flat[idx[: k // 10]] = np.nan
    flat[idx[k // 10: k // 10 + 2]] = np.inf
    flat[idx[k // 10 + 2: k // 10 + 4]] = -np.inf
    flat[idx[k // 10 + 4: k // 10 + 8]] = 0.0
    flat[idx[k // 10 + 8: k // 10 + 10]] = -0.0
    return x


def test_emu_trial_var_std_float32_bitwise(emu):
    rng = np.random.default_rng(3)
    x = (rng.normal(size=(9, 7, 13)) * 3 + 1).astype(np.float32)
    x[2, 1, 4] = np.nan
    trials = list(x)
    for take_sqrt in (0, 1):
        ref = (SO.trial_std if take_sqrt else SO.trial_var)(trials)
        for chunk in (None, 1, 4):
            got = emu_trial_var(emu, x, take_sqrt, chunk)
            assert np.array_equal(got, ref, equal_nan=True), (take_sqrt, chunk)


def test_emu_trial_var_complex(emu):
    rng = np.random.default_rng(4)
    x = (rng.normal(size=(7, 5, 11)) + 1j * rng.normal(size=(7, 5, 11))).astype(np.complex64)
    for take_sqrt in (0, 1):
        ref = (SO.trial_std if take_sqrt else SO.trial_var)(list(x))
        got = emu_trial_var(emu, x, take_sqrt)
        assert got.dtype == np.complex64 and np.all(got.imag == 0)
        assert_parity(got, ref, what="complex trial var")
        assert np.array_equal(emu_trial_var(emu, x, take_sqrt, 2), got)          # chunk-separable bit for bit


def test_emu_itc(emu):
    rng = np.random.default_rng(5)
    x = (rng.normal(size=(6, 2, 3, 9, 4)) + 1j * rng.normal(size=(6, 2, 3, 9, 4))).astype(np.complex64)
    x[:, 0, 1, 2, 3] = 0                                     # a zero bin in every trial
    got = emu_itc(emu, x, 1)
    ref = SO.itc(list(x), 1)
    assert got.shape == ref.shape == (2, 1, 9, 4)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[0, 0, 2, 3])
    ok = ~np.isnan(ref)
    assert_parity(got[ok], ref[ok], what="itc")
    assert np.array_equal(emu_itc(emu, x, 1, chunk=4), got, equal_nan=True)
    same = np.repeat(x[:1, :, :1], 5, axis=0)              # one taper: every unit vector the same
    one = emu_itc(emu, same, 1)
    assert np.nanmax(np.abs(one[~np.isnan(one)] - 1)) <= 1e-6


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape,axis", [((5, 40), 1), ((300, 3), 0), ((4, 200), 1), ((3, 17, 6), 1), ((2, 3, 150), 2)])
def test_emu_axis_var_std(emu, cplx, shape, axis):
    x = _edge(np.random.default_rng(6), shape, cplx)
    x[(0,) * (len(shape) - 1) + (slice(None),)] = np.nan    # one all-NaN slice along the last axis
    for op in ("var", "std"):
        got = emu_axis(emu, x, axis, op)
        ref = getattr(SO, "axis_" + op)(x, axis)
        assert got.dtype == x.dtype
        assert np.array_equal(np.isnan(got), np.isnan(ref)), op
        ok = np.isfinite(ref)
        assert_parity(got[ok], ref[ok], what=op)
        if cplx:
            assert np.all(got.imag[~np.isnan(got.real)] == 0)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape,axis", [((1, 1), 1), ((4, 2), 1), ((3, 3), 1), ((7, 11), 1), ((610, 2), 0),
                                        ((2, 599), 1), ((9000, 1), 0), ((3, 40, 5), 1), ((2, 33, 70), 2)])
def test_emu_axis_median_bitwise(emu, cplx, shape, axis):
    rng = np.random.default_rng(7)
    x = _edge(rng, shape, cplx) if x_size(shape) > 8 else rng.normal(size=shape).astype(np.float32)
    if cplx and x.dtype != np.complex64:
        x = (x + 1j * rng.normal(size=shape)).astype(np.complex64)
    if cplx and x.size > 8:                                  # ties in the real part: order by the imaginary part
        flat = x.reshape(-1)
        flat[1::3] = (np.round(flat[1::3].real) + 1j * flat[1::3].imag).astype(np.complex64)
        flat[2::3] = (np.round(flat[2::3].real) + 1j * flat[2::3].imag).astype(np.complex64)
    got = emu_axis(emu, x, axis, "median")
    ref = SO.axis_median(x, axis)
    assert got.dtype == x.dtype
    assert np.array_equal(got, ref, equal_nan=True)


def x_size(shape):
    return int(np.prod(shape))


def test_emu_median_all_nan_and_duplicates(emu):
    x = np.array([[np.nan, np.nan, np.nan], [2, 2, 5], [1, 2, 2], [3, np.nan, 1]], np.float32)
    assert np.array_equal(emu_axis(emu, x, 1, "median"), SO.axis_median(x, 1), equal_nan=True)
    y = np.array([[2, 2, 2, 9], [1, 1, 4, 4], [-0.0, 0.0, 0.0, -0.0]], np.float32)
    assert np.array_equal(emu_axis(emu, y, 1, "median"), SO.axis_median(y, 1))
    z = np.array([[1 + 1j, 1 + 0j, 4, 5]], np.complex64)
    assert emu_axis(emu, z, 1, "median")[0, 0] == np.complex64(2.5 + 0.5j)
