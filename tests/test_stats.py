"""spy.var / spy.std / spy.median / spy.itc without a GPU: the front end driven by the NumPy model (stats_oracle.py), its
argument checks, and a CPU emulation of the kernels of syncopy_amd/csrc/stats_kernel.h against NumPy."""
import ctypes as C
import os

import numpy as np
import pytest

import build_emu
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
    """the library's own launchers of csrc/stats.hip on the CPU.  ctx: default launch limits; few: 3 workgroups for the
    median, variance and transposition launches and 2 for the element-wise ones, so that every grid-stride loop runs"""
    lib = build_emu.emulated_library("stats")
    lib.ctx, lib.few = build_emu.ctx(lib), build_emu.ctx(lib, workgroups=3, elementwise_blocks=2)
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _split(shape, axis):
    return int(np.prod(shape[:axis])), shape[axis], int(np.prod(shape[axis + 1:]))


def _chunks(T, chunk):
    return [(a, min(chunk or T, T - a)) for a in range(0, T, chunk or T)]


def emu_trial_var(lib, x, take_sqrt, chunk=None, ctx=None):
    """spy.var / spy.std over trials as backend.py composes them: sums in chunks of trials, the mean, squared deviations
    in chunks, the finalisation"""
    ctx = ctx or lib.ctx
    x = np.ascontiguousarray(x)
    T, shape = x.shape[0], x.shape[1:]
    cplx, n = int(np.iscomplexobj(x)), int(np.prod(shape))
    mean = np.zeros(shape, x.dtype)
    acc = np.zeros(shape, np.float32)
    out = np.empty(shape, x.dtype)
    for a, k in _chunks(T, chunk):
        assert lib.spyhip_trial_sum(ctx, _p(x[a:]), _p(mean), k, n * (2 if cplx else 1)) == 0
    assert lib.spyhip_trial_sum_finalize(ctx, _p(mean), _p(mean), T, n, cplx) == 0
    for a, k in _chunks(T, chunk):
        assert lib.spyhip_trial_sqdev(ctx, _p(x[a:]), _p(mean), _p(acc), k, n, cplx) == 0
    assert lib.spyhip_trial_var_finalize(ctx, _p(acc), _p(out), T, n, cplx, int(take_sqrt)) == 0
    return out


def emu_itc(lib, x, taper_axis, chunk=None, ctx=None):
    ctx = ctx or lib.ctx
    x = np.ascontiguousarray(x, dtype=np.complex64)
    T, shape = x.shape[0], x.shape[1:]
    outer, K, inner = _split(shape, taper_axis)
    acc = np.zeros(shape, np.complex64)
    oshape = list(shape)
    oshape[taper_axis] = 1
    out = np.empty(oshape, np.float32)
    for a, k in _chunks(T, chunk):
        assert lib.spyhip_itc_accumulate(ctx, _p(x[a:]), _p(acc), k, outer * K * inner) == 0
    assert lib.spyhip_itc_finalize(ctx, _p(acc), _p(out), T, outer, K, inner) == 0
    return out


def emu_axis(lib, x, axis, op, ctx=None):
    """the median on 3 workgroups unless a context is given (each walks several slices when there are more)"""
    x = np.ascontiguousarray(x)
    outer, n, inner = _split(x.shape, axis)
    oshape = list(x.shape)
    oshape[axis] = 1
    out = np.empty(oshape, x.dtype)
    cplx = int(np.iscomplexobj(x))
    if op == "median":
        work = np.empty_like(x)
        assert lib.spyhip_axis_nanmedian(ctx or lib.few, _p(x), outer, n, inner, cplx, _p(work), _p(out)) == 0
    else:
        assert lib.spyhip_axis_nanvar(ctx or lib.ctx, _p(x), outer, n, inner, cplx, int(op == "std"), _p(out)) == 0
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("cplx", [False, True])
def test_emu_elementwise_grid_stride(emu, cplx):
    """1800 elements are 8 workgroups of 256: on 2 the trial and phase kernels walk their grid-stride loops"""
    rng = np.random.default_rng(8)
    x = rng.normal(size=(3, 2, 900)).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.normal(size=x.shape)).astype(np.complex64)
    for take_sqrt in (0, 1):
        emu.emu_launch_log_reset()
        ref = emu_trial_var(emu, x, take_sqrt, 2)
        assert set(build_emu.launches(emu)[:, 0]) == ({8, 15} if cplx else {8})
        got = emu_trial_var(emu, x, take_sqrt, 2, ctx=emu.few)
        assert set(build_emu.launches(emu)[:, 0]) == {2}
        assert np.array_equal(_bits(got), _bits(ref))
        assert_parity(got, (SO.trial_std if take_sqrt else SO.trial_var)(list(x)), what="trial var")
    if cplx:
        z = x.reshape(3, 2, 3, 300)
        ref = emu_itc(emu, z, 1, 2)
        got = emu_itc(emu, z, 1, 2, ctx=emu.few)
        assert set(build_emu.launches(emu)[:, 0]) == {8, 3, 2}
        assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("cplx", [False, True])
def test_emu_axis_workgroup_limit(emu, cplx):
    """more slices and tiles than workgroups: 1600 slices are 7 workgroups of the variance kernel, (7, 5, 2) along axis 1
    is 7 tiles of the transposition and 14 slices of the median - each on 3 workgroups, against the default limits"""
    rng = np.random.default_rng(9)
    x = _edge(rng, (40, 3, 40), cplx)
    for op in ("var", "std"):
        emu.emu_launch_log_reset()
        ref = emu_axis(emu, x, 1, op)
        got = emu_axis(emu, x, 1, op, ctx=emu.few)
        assert [int(g) for g in build_emu.launches(emu)[:, 0]] == [7, 3]
        assert np.array_equal(_bits(got), _bits(ref))
    y = _edge(rng, (7, 5, 2), cplx)
    emu.emu_launch_log_reset()
    ref = emu_axis(emu, y, 1, "median", ctx=emu.ctx)
    got = emu_axis(emu, y, 1, "median", ctx=emu.few)
    assert [int(g) for g in build_emu.launches(emu)[:, 0]] == [7, 14, 3, 3]
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.array_equal(got, SO.axis_median(y, 1), equal_nan=True)


def test_emu_refusals(emu):
    x = np.zeros((2, 3), np.float32)
    assert emu.spyhip_axis_nanmedian(emu.ctx, _p(x), 1, 2, 3, 0, None, _p(x)) == -1        # inner > 1 without a work buffer
    assert emu.spyhip_trial_sum_finalize(emu.ctx, _p(x), _p(x), 0, 6, 0) == -1             # no trial
