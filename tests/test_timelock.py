"""spy.timelockanalysis without a GPU: its argument checks, the front end driven by the NumPy model (timelock_oracle.py),
and a CPU emulation of the covariance kernels of syncopy_amd/csrc/cov_kernel.h against the model."""
import ctypes as C

import numpy as np
import pytest

import build_emu
import syncopy_amd as spy
import timelock_oracle as TO
from parity import assert_parity
from syncopy_amd._lib import SIGNATURES
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError

HOW = dict(compute_method="sequential", routine_classes=TO.TIMELOCK_OPS)


def _data(lengths=(300, 300, 300, 300), nchan=4, seed=0, fs=1000.0, offsets=None):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(sum(lengths), nchan)) + 2.0).astype(np.float32)
    e = np.concatenate([[0], np.cumsum(lengths)])
    off = np.full(len(lengths), -100.0) if offsets is None else np.asarray(offsets, dtype=float)
    return spy.AnalogData(x, samplerate=fs, trialdefinition=np.stack([e[:-1], e[1:], off], 1))


def cov_bound(ref):
    """one float32 rounding plus 1000 times the float64 dot-product error bound: 2^-23 |ref| + 1e-9 sqrt(ref_ii ref_jj)"""
    ref = np.asarray(ref, dtype=np.float64)
    d = np.sqrt(np.abs(np.diagonal(ref, axis1=-2, axis2=-1)))
    return 2.0 ** -23 * np.abs(ref) + 1e-9 * d[..., :, None] * d[..., None, :]


def assert_cov(got, ref, what=""):
    """`got` against the model's `ref` (both (..., C, C) float32): same NaNs, the parity criterion and cov_bound"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN mask"
    g, r = np.where(nan, 0, got).astype(np.float64), np.where(nan, 0, ref).astype(np.float64)
    worst = float((np.abs(g - r) / np.where(nan, 1.0, np.maximum(cov_bound(r), np.finfo(np.float64).tiny))).max())
    print(f"{what}: err/bound {worst:.3g}")
    assert worst <= 1.0, f"{what}: err/bound {worst:.3g}"
    assert_parity(g.astype(np.float32), r.astype(np.float32), what=what)


# ---- arguments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,exc", [
    (dict(ddof=-1), SPYValueError), (dict(ddof=1.5), SPYValueError), (dict(ddof="1"), SPYValueError),
    (dict(ddof=True), SPYValueError),
    (dict(covariance=1), SPYTypeError), (dict(covariance="yes"), SPYTypeError), (dict(covariance=None), SPYTypeError),
    (dict(keeptrials=0), SPYTypeError), (dict(keeptrials="no"), SPYTypeError),
    (dict(foo=1), SPYValueError), (dict(latency="always"), SPYValueError),
    (dict(trials=[0, 9]), SPYValueError),
    (dict(trials=[0, 1], select={"trials": [1, 2]}), SPYValueError),
    (dict(covariance=True, ddof=300), SPYValueError), (dict(covariance=True, ddof=1000), SPYValueError),
    (dict(latency=[5.0, 6.0]), SPYValueError),
])
def test_argument_errors(kw, exc):
    data = _data()
    with pytest.raises(exc):
        spy.timelockanalysis(data, **kw, **HOW)
    assert data.selection is None


def test_input_errors():
    with pytest.raises(SPYTypeError):
        spy.timelockanalysis(np.zeros((10, 2), dtype=np.float32), **HOW)
    with pytest.raises(SPYValueError):
        spy.timelockanalysis(spy.AnalogData(), **HOW)
    with pytest.raises(SPYValueError):
        spy.timelockanalysis(spy.AnalogData(np.zeros((2, 10), dtype=np.float32), samplerate=1.0, dimord=["channel", "time"]),
                             **HOW)
    with pytest.raises(SPYTypeError):
        spy.timelockanalysis(spy.AnalogData(np.zeros((10, 2)), samplerate=1.0), **HOW)
    prior = _data().selectdata({"trials": [0, 1]})
    with pytest.raises(SPYValueError):
        spy.timelockanalysis(prior, trials=[1], **HOW)
    assert prior.selection is not None and prior.selection.trial_ids == [0, 1]
    # no degree of freedom left: an error here, inf / NaN in the reference
    with pytest.raises(SPYValueError):
        spy.timelockanalysis(_data(lengths=(2, 2), offsets=(0, 0)), covariance=True, ddof=3, **HOW)
    # ... and ddof does not matter without the covariance
    assert spy.timelockanalysis(_data(lengths=(2, 2), offsets=(0, 0)), ddof=3, **HOW).cov is None


def test_accepted_and_ignored_kwargs():
    out = spy.timelockanalysis(_data(), parallel=False, chan_per_worker=2, **HOW)
    assert out.avg.shape == (300, 4)


# ---- the front end with the model ---------------------------------------------------------------------------------
def test_defaults_shapes_and_metadata():
    data = _data()
    data.cfg = {"earlier": {"a": 1}}
    tld = spy.timelockanalysis(data, **HOW)
    assert isinstance(tld, spy.TimeLockData) and tld.dimord == ["time", "channel"]
    assert tld.data.dtype == np.float32 and np.array_equal(tld.data, data.data)
    assert np.array_equal(tld.trialdefinition, data.trialdefinition)
    assert len(tld.trials) == 4 and np.array_equal(tld.trials[2], data.trials[2])
    assert np.array_equal(tld.time[1], data.time[1])
    assert list(tld.channel) == list(data.channel) and tld.samplerate == 1000.0
    assert tld.avg.shape == tld.var.shape == (300, 4) and tld.avg.dtype == tld.var.dtype == np.float32
    assert np.array_equal(tld.avg, spy.mean(data, dim="trials", **dict(HOW, routine_classes=TO.STATS_OPS)).data)
    assert np.array_equal(tld.var, TO.STATS_OPS["trial_var"](data.trials))
    assert tld.cov is None and data.selection is None
    assert tld.cfg["earlier"] == {"a": 1}
    assert tld.cfg["timelockanalysis"] == dict(latency="maxperiod", covariance=False, ddof=None, trials="all",
                                               keeptrials=False)
    empty = spy.TimeLockData()
    assert empty.avg is None and empty.var is None and empty.cov is None and empty.data is None


@pytest.mark.parametrize("ddof", [None, 0, 3])
def test_covariance_keeptrials_both_ways(ddof):
    data = _data(nchan=5, seed=1)
    per = [np.cov(x, ddof=ddof, rowvar=False).astype(np.float32) for x in data.trials]
    kept = spy.timelockanalysis(data, covariance=True, ddof=ddof, keeptrials=True, **HOW)
    assert kept.cov.shape == (4, 5, 5) and kept.cov.dtype == np.float32
    assert np.array_equal(kept.cov, np.stack(per))
    avg = spy.timelockanalysis(data, covariance=True, ddof=ddof, **HOW)
    acc = np.zeros((5, 5), dtype=np.float32)
    for c in per:
        acc += c
    acc /= 4
    assert avg.cov.shape == (5, 5) and avg.cov.dtype == np.float32 and np.array_equal(avg.cov, acc)
    assert np.array_equal(avg.cov, TO.cov_average(per))
    assert avg.cfg["timelockanalysis"]["ddof"] == ddof and avg.cfg["timelockanalysis"]["covariance"] is True


def test_squeeze_with_one_trial_and_one_channel():
    one_trial = _data(lengths=(300,), nchan=3)
    assert spy.timelockanalysis(one_trial, covariance=True, keeptrials=True, **HOW).cov.shape == (3, 3)
    assert spy.timelockanalysis(one_trial, covariance=True, **HOW).cov.shape == (3, 3)
    one_chan = _data(nchan=1)
    kept = spy.timelockanalysis(one_chan, covariance=True, keeptrials=True, **HOW)
    assert kept.cov.shape == (4,)
    assert np.array_equal(kept.cov, [np.float32(np.var(x[:, 0].astype(np.float64), ddof=1)) for x in one_chan.trials])
    assert spy.timelockanalysis(one_chan, covariance=True, **HOW).cov.shape == ()
    picked = spy.timelockanalysis(_data(), covariance=True, keeptrials=True, select={"channel": [2]}, **HOW)
    assert picked.cov.shape == (4,) and list(picked.channel) == ["channel3"]


def test_latency_keywords_and_window():
    # trial time axes: [-0.1, 0.199], [-0.05, 0.249], [-0.1, 0.199]
    data = _data(lengths=(300, 300, 300), offsets=(-100, -50, -100), seed=2)
    tr = data.trials
    cases = {
        "maxperiod": [(0, 300, -100), (0, 300, -50), (0, 300, -100)],
        "minperiod": [(50, 300, -50), (0, 250, -50), (50, 300, -50)],          # [-0.05, 0.199]
        "poststim": [(100, 300, 0), (50, 300, 0), (100, 300, 0)],              # [0, 0.249]
    }
    for latency, cuts in cases.items():
        if len({b - a for a, b, _ in cuts}) != 1:
            with pytest.raises(SPYValueError):                                # unequal lengths after the cut
                spy.timelockanalysis(data, latency=latency, **HOW)
            continue
        tld = spy.timelockanalysis(data, latency=latency, covariance=True, **HOW)
        cut = [tr[k][a:b] for k, (a, b, _) in enumerate(cuts)]
        n = cuts[0][1] - cuts[0][0]
        assert np.array_equal(tld.data, np.concatenate(cut)), latency
        assert np.array_equal(tld.trialdefinition, [[k * n, (k + 1) * n, off] for k, (_, _, off) in enumerate(cuts)]), latency
        assert np.array_equal(tld.avg, TO.STATS_OPS["trial_mean"](cut)) and tld.avg.shape == (n, 4)
        assert np.array_equal(tld.var, TO.STATS_OPS["trial_var"](cut))
        assert np.array_equal(tld.cov, TO.cov_average([TO.cov(x) for x in cut]))
    assert data.selection is None
    # prestim [-0.1, 0]: 101, 51 and 101 samples - equal once the middle trial is left out
    with pytest.raises(SPYValueError):
        spy.timelockanalysis(data, latency="prestim", **HOW)
    tld = spy.timelockanalysis(data, latency="prestim", trials=[0, 2], **HOW)
    assert np.array_equal(tld.data, np.concatenate([tr[0][:101], tr[2][:101]]))
    assert np.array_equal(tld.trialdefinition, [[0, 101, -100], [101, 202, -100]])
    # poststim on equal offsets, and a window
    same = _data(seed=3)
    tld = spy.timelockanalysis(same, latency="poststim", **HOW)
    assert np.array_equal(tld.data, np.concatenate([x[100:] for x in same.trials]))
    tld = spy.timelockanalysis(same, latency=[-0.02, 0.05], covariance=True, keeptrials=True, **HOW)
    cut = [x[80:151] for x in same.trials]
    assert np.array_equal(tld.data, np.concatenate(cut)) and tld.avg.shape == (71, 4)
    assert np.array_equal(tld.trialdefinition[:, 2], [-20] * 4)
    assert np.array_equal(tld.cov, np.stack([TO.cov(x) for x in cut]))
    assert np.array_equal(tld.time[0], (np.arange(71) - 20) / 1000.0)


def test_unequal_lengths_raise():
    with pytest.raises(SPYValueError, match="same shape"):
        spy.timelockanalysis(_data(lengths=(300, 200, 300)), **HOW)


def test_trials_keyword_select_and_restored_selection():
    data = _data(nchan=6, seed=4)
    a = spy.timelockanalysis(data, trials=[3, 1], covariance=True, **HOW)
    b = spy.timelockanalysis(data, select={"trials": [3, 1]}, covariance=True, **HOW)
    for name in ("data", "avg", "var", "cov", "trialdefinition"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.data, np.concatenate([data.trials[3], data.trials[1]]))
    assert a.cfg["timelockanalysis"]["trials"] == [3, 1] and "select" not in a.cfg["timelockanalysis"]
    assert b.cfg["timelockanalysis"]["select"] == {"trials": [3, 1]}
    # a prior selection of channels takes the trials keyword and the latency on top, and is there again afterwards
    data.selectdata({"channel": [4, 0, 2]})
    prior = data.selection
    c = spy.timelockanalysis(data, trials=[2, 0], latency=[0.0, 0.1], covariance=True, keeptrials=True, **HOW)
    assert data.selection is prior
    cut = [data.trials[k][100:201][:, [4, 0, 2]] for k in (2, 0)]
    assert np.array_equal(c.data, np.concatenate(cut)) and list(c.channel) == list(data.channel[[4, 0, 2]])
    assert np.array_equal(c.cov, np.stack([TO.cov(x) for x in cut]))
    assert np.array_equal(c.avg, TO.STATS_OPS["trial_mean"](cut))
    # a prior latency is replaced
    data.selectdata({"trials": [1, 2], "latency": [0.0, 0.01]})
    d = spy.timelockanalysis(data, **HOW)
    assert d.avg.shape == (300, 6) and data.selection.select == {"trials": [1, 2], "latency": [0.0, 0.01]}
    # also when the call fails
    with pytest.raises(SPYValueError):
        spy.timelockanalysis(data, trials=[0], **HOW)
    assert data.selection.select == {"trials": [1, 2], "latency": [0.0, 0.01]}


def test_container_still_refused(tmp_path):
    tld = spy.timelockanalysis(_data(), **HOW)
    with pytest.raises(SPYTypeError):
        spy.save(tld, filename=str(tmp_path / "x.timelock"))
    with pytest.raises(SPYValueError):
        spy.load(str(tmp_path / "x.timelock"))


# ---- CPU emulation of cov_kernel.h --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    """the library's own launcher of csrc/cov.hip on the CPU, with a context of default launch limits"""
    lib = build_emu.emulated_library("cov")
    lib.emu_cov_small.restype, lib.emu_cov_small.argtypes = SIGNATURES["spyhip_cov_f32"]
    lib.ctx = build_emu.ctx(lib)
    return lib


def _run(emu, x, ddof, fn=None, ctx=None, waves=2):
    """(covariances, column means) of the launcher `fn` (default: the one with 2 waves per mean); the grids of the two
    kernels are read from the launch log"""
    T, N, Cn = x.shape
    ctx = ctx or emu.ctx
    out = np.full((T, Cn, Cn), -7.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    emu.emu_launch_log_reset()
    assert (fn or emu.emu_cov_small)(ctx, p(x), p(out), T, N, Cn, 1 if ddof is None else ddof) == 0
    g = build_emu.launches(emu)
    nb = -(-Cn // 64)
    assert np.all(g[1::2, 0] == nb * (nb + 1) // 2)                     # workgroups of the covariance kernel per trial
    assert np.all(g[0::2, 0] == nb) and np.all(g[0::2, 3] == 64 * waves) and g[:, 1].sum() == 2 * T
    per = g[0, 1]                                                       # trials of a launch: the means of the last one
    mean = np.ctypeslib.as_array(C.cast(emu.emu_ctx_scratch(ctx), C.POINTER(C.c_double)), (per, Cn))[:g[-1, 1]].copy()
    return out, mean


def _batch(T, N, Cn, seed, dc=0.0):
    """channel scales from 1e-2 to 1e2, correlated channels, a mean of its own per channel"""
    rng = np.random.default_rng(seed)
    mix = rng.normal(size=(Cn, Cn)) / np.sqrt(Cn) + np.eye(Cn)
    x = rng.normal(size=(T, N, Cn)) @ mix
    x = x * np.logspace(-2, 2, Cn)[rng.permutation(Cn)] + rng.normal(size=(T, 1, Cn)) + dc
    return np.ascontiguousarray(x, dtype=np.float32)


# n = 2 leaves no degree of freedom at ddof 3: np.cov gives inf / NaN there and the front end refuses it (test_input_errors)
EMU_CASES = [(c, n, d) for c in (1, 5, 16, 33, 70) for n in (2, 257, 1000) for d in (None, 0, 3) if n - (1 if d is None else d) > 0]


@pytest.mark.parametrize("nchan,n,ddof", EMU_CASES)
def test_emu_cov(emu, nchan, n, ddof):
    x = _batch(2, n, nchan, seed=nchan + n)
    got, mean = _run(emu, x, ddof)
    assert np.allclose(mean, x.astype(np.float64).mean(axis=1), rtol=1e-13, atol=0)
    for t in range(2):
        assert_cov(got[t], TO.cov(x[t], ddof), what=f"cov c={nchan} n={n} ddof={ddof} trial {t}")
        assert np.array_equal(got[t], got[t].T)


def test_emu_cov_dc_offset(emu):
    x = _batch(1, 257, 33, seed=5, dc=1e4)
    got, _ = _run(emu, x, None)
    assert_cov(got[0], TO.cov(x[0]), what="cov with a DC offset of 1e4")


def test_emu_cov_nan_stays_in_its_row_and_column(emu):
    x = _batch(3, 257, 70, seed=6)
    x[1, 100, 66] = np.nan
    x[2, 0, 3] = np.nan
    x[2, 256, 64] = np.nan
    got, _ = _run(emu, x, None)
    for t, bad in ((0, []), (1, [66]), (2, [3, 64])):
        mask = np.zeros((70, 70), dtype=bool)
        mask[bad, :] = True
        mask[:, bad] = True
        assert np.array_equal(np.isnan(got[t]), mask), t
        assert_cov(got[t], TO.cov(x[t]), what=f"NaN trial {t}")


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("n,nchan", [(33, 65), (8, 1)])
def test_emu_cov_library_waves(emu, n, nchan, ddof):
    """8 waves per mean, as the library launches: more waves than rows (8, 1), and rows that do not divide by them"""
    x = _batch(2, n, nchan, seed=nchan + n)
    got, mean = _run(emu, x, ddof, fn=emu.spyhip_cov_f32, waves=8)
    assert np.allclose(mean, x.astype(np.float64).mean(axis=1), rtol=1e-13, atol=0)
    for t in range(2):
        assert_cov(got[t], TO.cov(x[t], ddof), what=f"cov c={nchan} n={n} ddof={ddof} trial {t}")
        assert np.array_equal(got[t], got[t].T)


def test_emu_cov_trial_chunks_and_refusals(emu):
    """7 trials at 3 per launch: the offsets of input, output and the mean scratch in the loop over grid.y"""
    x = _batch(7, 33, 65, seed=8)
    ref, _ = _run(emu, x, 1, fn=emu.spyhip_cov_f32, waves=8)
    few = build_emu.ctx(emu, grid_yz=3)
    got, mean = _run(emu, x, 1, fn=emu.spyhip_cov_f32, ctx=few, waves=8)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.allclose(mean, x[6:].astype(np.float64).mean(axis=1), rtol=1e-13, atol=0)     # the last launch: trial 6
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    for ddof in (33, 34):                                                                   # ddof >= n
        assert emu.spyhip_cov_f32(emu.ctx, p(x), p(got), 7, 33, 65, ddof) == -1
    assert emu.spyhip_cov_f32(emu.ctx, p(x), p(x), 7, 33, 65, 1) == -1                      # in == out
