"""The Hilbert option of spy.preprocessing on the device (csrc/hilbert.hip): backend.hilbert on raw tensors against the
float64 oracle (hilbert_oracle.py) at the shared parity criterion, and spy.preprocessing on the device against the model
table through the same front end.  `angle` is compared as abs(oracle) exp(i angle) against the oracle's analytic signal:
a phase near the +-pi cut or at a vanishing amplitude is weighed by its amplitude, and no element is left out.

Measured on an MI355X: see DESIGN.md section 8."""
import importlib

import numpy as np
import pytest

import hilbert_oracle as HO
import syncopy_amd as spy
from parity import excess
from syncopy_amd.shared.errors import SPYValueError
from test_hilbert import EMU_LENGTHS, route  # noqa: F401  (the route fixture: csrc/hilbert_route.h through its shim)

pytestmark = pytest.mark.gpu
HOW = dict(compute_method="sequential", routine_classes=HO.HILBERT_OPS)
FS = 1000.0
LENGTHS = sorted({n for fam in EMU_LENGTHS.values() for n in fam} | {1, 8192, 8193, 16384})


def _run(x, output):
    import torch
    from syncopy_amd import backend
    xd = torch.from_numpy(x).cuda()
    out = torch.full(x.shape, -7.0, dtype=torch.complex64 if output == "complex" else torch.float32, device="cuda")
    flag = torch.zeros(x.shape[0], dtype=torch.int32, device="cuda")
    backend.hilbert(xd, out, output, flag)
    torch.cuda.synchronize()
    return out.cpu().numpy(), flag.cpu().numpy()


def _x(n, nchan, ntrials=3):
    return (np.random.default_rng(7 * n + nchan).normal(size=(ntrials, n, nchan)) + 2.0).astype(np.float32)


def _check(got, z, output, what):
    """`z`: the oracle's analytic signal (complex128)"""
    if output == "angle":
        got, ref = np.abs(z) * np.exp(1j * got.astype(np.float64)), z
    else:
        assert got.dtype == (np.complex64 if output == "complex" else np.float32)
        ref = HO.CONVERSIONS[output](z)
    e = excess(got, ref)
    print(f"{what}: err/tol {e:.3g}")
    assert e <= 1.0, f"{what}: err/tol {e:.3g}"


@pytest.mark.parametrize("n", LENGTHS)
def test_backend_lengths(n):
    for nchan in (1, 5, 65):
        x = _x(n, nchan)
        got, flag = _run(x, "complex")
        assert not flag.any() and np.array_equal(got.real, x)
        _check(got, HO.analytic64(x), "complex", f"N={n}, {nchan} channels")


@pytest.mark.parametrize("n", [256, 1000, 4100])
def test_backend_outputs(n):
    x = _x(n, 5)
    z = HO.analytic64(x)
    for output in HO.OUTPUTS:
        got, _ = _run(x, output)
        _check(got, z, output, f"N={n}, {output}")


def test_backend_longest_trial():
    """2^20 samples: every index of the complex128 passes at their longest"""
    x = _x(1 << 20, 2, ntrials=1)
    got, flag = _run(x, "imag")
    assert not flag.any()
    _check(got, HO.analytic64(x), "imag", "N=2^20")


@pytest.mark.parametrize("n", [1, 17, 4096, 4097])
def test_kernel_name_is_the_route(route, n):
    from syncopy_amd import backend
    assert backend.hilbert_plan(n).kernel_name == route(n)["text"]


def test_beyond_2_pow_20_is_refused_before_any_device_work():
    import torch
    from syncopy_amd import backend
    n = (1 << 20) + 1
    xd = torch.zeros((1, n, 1), dtype=torch.float32, device="cuda")
    out = torch.full_like(xd, 7.0)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(backend.SpyHipError, match=r"2\^20"):
        backend.hilbert(xd, out, "abs", flag)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and not flag.any().item()
    trl = np.array([[0, n, 0]])
    with pytest.raises(SPYValueError, match="Hilbert"):
        spy.preprocessing(spy.AnalogData(np.zeros((n, 1), dtype=np.float32), samplerate=FS, trialdefinition=trl),
                          filter_class=None, polyremoval=0, hilbert="abs")


# ---- through spy.preprocessing, device against model -----------------------------------------------------------------
def _data(lengths, nchan, seed=0):
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    x = rng.normal(size=(total, nchan)) + rng.normal(size=(1, nchan)) + 2.0
    edges = np.concatenate([[0], np.cumsum(lengths)])
    trl = np.stack([edges[:-1], edges[1:], np.zeros(len(lengths))], axis=1)
    return spy.AnalogData(x.astype(np.float32), samplerate=FS, trialdefinition=trl)


def _compare(data, what, **kw):
    """The device against the model through the same front end: the same NaN pattern, nan_trials, labels and trial
    definition, the finite elements at parity per trial (`angle`: weighed by the model's analytic signal)."""
    got = spy.preprocessing(data, **kw)
    ref = spy.preprocessing(data, **kw, **HOW)
    assert got.data.dtype == ref.data.dtype and got.data.shape == ref.data.shape, what
    assert got.data.dtype == (np.complex64 if kw["hilbert"] == "complex" else np.float32), what
    assert np.array_equal(np.asarray(got.trialdefinition), np.asarray(ref.trialdefinition)), what
    assert list(got.channel) == list(ref.channel), what
    assert got.info.get("nan_trials") == ref.info.get("nan_trials"), what
    assert got.cfg["preprocessing"] == ref.cfg["preprocessing"], what
    refs = ref.trials
    if kw["hilbert"] == "angle":
        refs = spy.preprocessing(data, **dict(kw, hilbert="complex"), **HOW).trials
    worst = 0.0
    for g, r in zip(got.trials, refs):
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN pattern"
        ok = ~np.isnan(r)
        if not ok.any():
            continue
        if kw["hilbert"] == "angle":
            worst = max(worst, excess(np.abs(r[ok]) * np.exp(1j * g[ok].astype(np.float64)), r[ok].astype(np.complex128)))
        else:
            worst = max(worst, excess(g[ok], r[ok].astype(np.complex128 if np.iscomplexobj(r) else np.float64)))
    print(f"{what}: err/tol {worst:.3g}")
    assert worst <= 1.0, f"{what}: err/tol {worst:.3g}"
    return got, ref


@pytest.mark.parametrize("output", HO.OUTPUTS)
def test_front_end_outputs(output):
    _compare(_data([256, 256, 256], 6), f"hilbert={output}", filter_class=None, polyremoval=0, hilbert=output)


def test_front_end_bandpass_chain():
    _compare(_data([1000, 1000], 5, seed=1), "bp + abs", filter_type="bp", freq=[20, 80], hilbert="abs")


def test_front_end_unequal_lengths_and_selection():
    data = _data([300, 200, 300], 8, seed=2)
    _compare(data, "unequal", filter_class=None, polyremoval=1, hilbert="complex")
    _compare(data, "unequal, selection", filter_class=None, polyremoval=1, hilbert="imag",
             select={"trials": [2, 0, 1], "channel": [5, 1, 6]})


def test_front_end_two_chunks(monkeypatch):
    mod = importlib.import_module("syncopy_amd.preproc.preprocessing")
    data = _data([500, 300, 500, 300, 500], 6, seed=3)
    for output in ("abs", "complex"):
        kw = dict(filter_class=None, polyremoval=0, hilbert=output)
        full, _ = _compare(data, f"chunks, {output}", **kw)
        monkeypatch.setattr(mod, "CHUNK_BYTES", 2 * 500 * 6 * 4)       # the three trials of 500 samples in two launches
        small = spy.preprocessing(data, **kw)
        monkeypatch.undo()
        assert np.array_equal(full.data, small.data), output


@pytest.mark.parametrize("n", [256, 300], ids=["packed", "bluestein"])
def test_front_end_nan_in_one_channel(n):
    data = _data([n, n, n], 6, seed=4)
    data.data[n + n // 2, 1] = np.nan
    with pytest.warns(UserWarning, match="NaN"):
        got, _ = _compare(data, f"NaN, N={n}", filter_class=None, polyremoval=0, hilbert="abs")
    assert got.info["nan_trials"] == [1]
    assert np.isnan(got.trials[1][:, 1]).all() and np.isnan(got.data).sum() == n
