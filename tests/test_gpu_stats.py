"""spy.var / spy.std / spy.median / spy.itc on the device (csrc/stats.hip) against the NumPy model of the reference
(stats_oracle.py) run through the same front end."""
import os

import numpy as np
import pytest

import syncopy_amd as spy
import stats_oracle as SO
from parity import assert_parity

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "mean_variants.npz"))
HOW = dict(compute_method="sequential", routine_classes=SO.STATS_OPS)


def _analog():
    return spy.AnalogData(np.concatenate(list(Z["data"])), samplerate=float(Z["samplerate"]),
                          trialdefinition=Z["trialdefinition"])


def _spectral(key):
    s = spy.SpectralData(Z[key], samplerate=float(Z["samplerate"]), trialdefinition=Z["spec_trldef"])
    s.channel = np.array(["channel%d" % (i + 1) for i in range(Z[key].shape[-1])])
    return s


def _make(src):
    return _analog() if src == "analog" else _spectral(src)


def _check(got, ref, op, dim, what):
    assert got.data.shape == ref.data.shape and got.data.dtype == ref.data.dtype, what
    g, r = got.data, ref.data
    if op == "median":
        assert np.array_equal(g, r, equal_nan=True), what
        return
    if np.iscomplexobj(g):
        assert np.all(g.imag[~np.isnan(g.real)] == 0), what
    if dim == "trials" and not np.iscomplexobj(g):
        assert np.array_equal(g, r, equal_nan=True), what          # the reference's rounding sequence, bit for bit
        return
    ok = np.isfinite(r)
    assert np.array_equal(ok, np.isfinite(g)), what
    assert_parity(g[ok], r[ok], what=what)
    if ok.any():
        assert np.abs(g[ok] - r[ok]).max() <= 1e-6 * np.abs(r[ok]).max(), what


SEL = {"analog": {"trials": [0, 2, 3], "channel": [0, 3]}, "spec": {"trials": [1, 4, 5], "channel": [1, 2, 4]},
       "pow": {"trials": [5, 0]}}


@pytest.mark.parametrize("op", ["var", "std", "median"])
@pytest.mark.parametrize("src", ["analog", "spec", "pow"])
def test_device_stats_every_dim(op, src):
    data = _make(src)
    fn = getattr(spy, op)
    dims = ([] if op == "median" else ["trials"]) + list(data.dimord)
    for dim in dims:
        for keeptrials in ((True,) if dim == "trials" else (True, False)):
            for select in (None, SEL[src]):
                kw = dict(dim=dim, keeptrials=keeptrials, select=select)
                what = f"{op} {src} {kw}"
                got = fn(data, **kw)
                ref = fn(data, **kw, **HOW)
                _check(got, ref, op, dim, what)
                assert np.array_equal(np.asarray(got.trialdefinition, float), np.asarray(ref.trialdefinition, float)), what
                if dim != "trials" and dim != "time":
                    assert getattr(got, dim, None) is None or list(getattr(got, dim)) == [op], what


def _edge_data(rng, shape, cplx):
    x = rng.normal(size=shape).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.normal(size=shape)).astype(np.complex64)
        flat = x.reshape(-1)
        flat[::4] = (np.round(flat[::4].real) + 1j * flat[::4].imag).astype(np.complex64)   # ties in the real part
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)
    k = flat.size // 10
    flat[idx[:k]] = np.nan
    flat[idx[k:k + 3]] = np.inf
    flat[idx[k + 3:k + 6]] = -np.inf
    flat[idx[k + 6:k + 12]] = 0.0
    flat[idx[k + 12:k + 18]] = -0.0
    return x


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape,axis", [((1, 4), 0), ((2, 3), 0), ((3, 5), 0), ((599, 3), 0), ((600, 2), 0),
                                        ((601, 3), 0), ((7, 1200), 1), ((100000, 2), 0), ((3, 100000), 1),
                                        ((40, 9000), 1), ((5, 33, 70), 1)] +
                         # MED_STAGE_BYTES = 32768: a slice's keys stay in LDS up to 8192 float32 / 4096 complex64 elements
                         [(s, a) for n in (4095, 4096, 4097, 8191, 8192, 8193) for s, a in (((n, 3), 0), ((3, n), 1))])
def test_device_axis_edge_slices(cplx, shape, axis):
    import torch
    from syncopy_amd import backend
    rng = np.random.default_rng(sum(shape) + axis)
    x = _edge_data(rng, shape, cplx)
    sl = [slice(None)] * len(shape)
    sl[1 - axis if len(shape) == 2 else 0] = 0
    x[tuple(sl)] = np.nan                                  # one all-NaN slice
    d = torch.from_numpy(x).cuda()
    med = backend.axis_nanmedian(d, axis).cpu().numpy()
    assert np.array_equal(med, SO.axis_median(x, axis), equal_nan=True)
    for take_sqrt, ref in ((False, SO.axis_var(x, axis)), (True, SO.axis_std(x, axis))):
        got = backend.axis_nanvar(d, axis, take_sqrt).cpu().numpy()
        ok = np.isfinite(ref)
        assert np.array_equal(ok, np.isfinite(got))
        assert_parity(got[ok], ref[ok], what=f"axis var {shape} {axis}")
        if cplx:
            assert np.all(got.imag[~np.isnan(got.real)] == 0)


def test_device_median_is_reproducible_and_handles_small_counts():
    import torch
    from syncopy_amd import backend
    x = np.array([[np.nan, np.nan, 2], [1, 1, 4], [3, -1, np.inf], [-0.0, 0.0, 0.0]], np.float32)
    got = backend.axis_nanmedian(torch.from_numpy(x).cuda(), 1).cpu().numpy()
    assert np.array_equal(got, SO.axis_median(x, 1), equal_nan=True)
    z = np.array([[1 + 1j, 1 + 0j, 4, 5]], np.complex64)
    assert backend.axis_nanmedian(torch.from_numpy(z).cuda(), 1).cpu().numpy()[0, 0] == np.complex64(2.5 + 0.5j)
    big = torch.from_numpy(np.random.default_rng(1).normal(size=(64, 5000)).astype(np.float32)).cuda()
    a = backend.axis_nanmedian(big, 1).cpu().numpy()
    b = backend.axis_nanmedian(big, 1).cpu().numpy()
    assert np.array_equal(a, b)


def test_device_trial_moments_chunk_invariance(monkeypatch):
    from syncopy_amd.statistics import summary_stats
    rng = np.random.default_rng(2)
    x = rng.normal(size=(9 * 64, 7)).astype(np.float32)
    x[5, 3] = np.nan
    data = spy.AnalogData(x, samplerate=100.0, trialdefinition=np.array([[64 * t, 64 * (t + 1), 0] for t in range(9)]))
    spec = _spectral("spec")
    full = [spy.var(data, dim="trials").data, spy.std(data, dim="trials").data, spy.std(spec, dim="trials").data,
            spy.itc(spec).data]
    assert np.array_equal(full[0], spy.var(data, dim="trials", **HOW).data, equal_nan=True)
    monkeypatch.setattr(summary_stats, "CHUNK_BYTES", 1)      # one trial per upload
    small = [spy.var(data, dim="trials").data, spy.std(data, dim="trials").data, spy.std(spec, dim="trials").data,
             spy.itc(spec).data]
    for a, b in zip(full, small):
        assert np.array_equal(a, b, equal_nan=True)


def _fourier(data, **kw):
    return spy.freqanalysis(data, output="fourier", keeptrials=True, **kw)


@pytest.mark.parametrize("kw", [dict(method="mtmfft", keeptapers=True, tapsmofrq=4),
                                dict(method="mtmconvol", taper="hann", t_ftimwin=0.128, toi="all")])
def test_device_itc_end_to_end(kw):
    data = spy.synthdata.ar2_network(AdjMat=np.zeros((4, 4)), nSamples=1000, nTrials=12, seed=3)
    spec = _fourier(data, **kw)
    got = spy.itc(spec)
    ref = spy.itc(spec, **HOW)
    assert got.data.dtype == np.float32 and got.data.shape == ref.data.shape
    assert got.data.shape[spec.dimord.index("taper")] == 1
    assert got.data.shape[0] == spec.data.shape[0] // len(spec.trials)
    zero = np.zeros(ref.data.shape, bool)
    for trl in spec.trials:
        zero |= np.any(np.asarray(trl) == 0, axis=1, keepdims=True)
    assert np.array_equal(np.isnan(got.data), np.isnan(ref.data))
    assert np.array_equal(np.isnan(got.data), zero)
    ok = ~np.isnan(ref.data)
    assert_parity(got.data[ok], ref.data[ok], what=f"itc {kw['method']}")
    assert np.all((got.data[ok] >= 0) & (got.data[ok] <= 1 + 1e-6))


def test_device_itc_of_repeated_trial_is_one():
    one = spy.synthdata.ar2_network(AdjMat=np.zeros((3, 3)), nSamples=500, nTrials=1, seed=9)
    x = np.asarray(one.trials[0])
    rep = spy.AnalogData(np.concatenate([x] * 7), samplerate=one.samplerate,
                         trialdefinition=np.array([[500 * t, 500 * (t + 1), 0] for t in range(7)]))
    spec = _fourier(rep, method="mtmfft", taper="hann")
    got = spy.itc(spec).data
    ok = ~np.isnan(got)
    assert ok.any() and np.abs(got[ok] - 1).max() <= 1e-6


def test_device_float64_is_refused():
    from syncopy_amd.shared.errors import SPYTypeError
    f64 = spy.AnalogData(np.zeros((30, 2)), samplerate=10.0, trialdefinition=np.array([[0, 15, 0], [15, 30, 0]]))
    for fn in (spy.var, spy.std, spy.median):
        with pytest.raises(SPYTypeError):
            fn(f64, dim="time")
