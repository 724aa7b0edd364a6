"""spy.resampledata without a GPU: the NumPy / SciPy model (resample_oracle.py) with the package's filter design against
recorded results of the reference's resampling module, the front end driven by the model, its argument checks, and a
CPU emulation of the kernel of syncopy_amd/csrc/resample_kernel.h against the model."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import build_emu
import syncopy_amd as spy
import resample_oracle as RO
from parity import assert_parity, excess
from syncopy_amd._lib import SIGNATURES
from syncopy_amd.preproc import design
from syncopy_amd.shared.errors import SPYTypeError, SPYValueError

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "resample.npz"))
HOW = dict(compute_method="sequential", routine_classes=RO.RESAMPLE_OPS)


def _data(lengths=(300, 200, 300), nchan=4, seed=0, fs=1000.0, offsets=None):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(sum(lengths), nchan)) + 2.0).astype(np.float32)
    e = np.concatenate([[0], np.cumsum(lengths)])
    off = np.zeros(len(lengths)) if offsets is None else np.asarray(offsets, dtype=float)
    return spy.AnalogData(x, samplerate=fs, trialdefinition=np.stack([e[:-1], e[1:], off], 1))


def golden_cases():
    for name in G["names"]:
        fs, new_fs, order, lpfreq = G[f"{name}_par"]
        yield str(name), fs, new_fs, (None if order < 0 else int(order)), (None if lpfreq < 0 else float(lpfreq))


def model_of_case(x, fs, new_fs, order, lpfreq):
    """the contract, step by step, with the package's own design"""
    frac = Fraction.from_float(new_fs / fs).limit_denominator()
    up, down = frac.numerator, frac.denominator
    f_c = 0.5 * new_fs / fs if lpfreq is None else lpfreq / fs
    taps = design.windowed_sinc("hamming", order, f_c / up) * up
    return RO.resample(x, taps, up, down), up, down


# ---- model and design against the reference's recorded results ----------------------------------------------------
def test_model_matches_recorded_reference():
    seen = set()
    for name, fs, new_fs, order, lpfreq in golden_cases():
        x, ref = G[f"{name}_in"], G[f"{name}_out"]
        if name.startswith("d"):
            got = RO.downsample(x, int(fs // new_fs))
            assert np.array_equal(got, ref), name
            continue
        got, up, down = model_of_case(x, fs, new_fs, order, lpfreq)
        seen.add((up, down))
        assert got.shape == ref.shape == (-(-x.shape[0] * up // down), x.shape[1]), name
        e = excess(got, ref)
        print(f"{name}: up {up} down {down} err/tol {e:.3g}")
        assert e <= 1.0, f"{name}: err/tol {e:.3g}"
    assert seen == {(3, 5), (333, 1000), (441, 1000), (999, 1000), (3, 4), (1, 30)}


@pytest.mark.parametrize("name,fs,new_fs,order,lpfreq", list(golden_cases()))
def test_front_end_matches_recorded_reference(name, fs, new_fs, order, lpfreq):
    x = G[f"{name}_in"]
    data = spy.AnalogData(x.copy(), samplerate=fs)
    kw = dict(method="downsample") if name.startswith("d") else dict(order=order, lpfreq=lpfreq)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = spy.resampledata(data, resamplefs=new_fs, **kw, **HOW)
    assert out.data.dtype == np.float32 and out.samplerate == new_fs
    assert_parity(out.data, G[f"{name}_out"], what=name)


# ---- the front end with the model ---------------------------------------------------------------------------------
def test_defaults_lengths_and_trialdefinition():
    data = _data(lengths=(300, 200, 301), offsets=(-100, 0, 33))
    data.cfg = {"earlier": {"a": 1}}
    out = spy.resampledata(data, resamplefs=600, **HOW)
    taps = design.windowed_sinc("hamming", 200, 0.3 / 3) * 3                 # order = shortest trial, up 3, down 5
    for g, x, n in zip(out.trials, data.trials, (180, 120, 181)):
        assert g.shape == (n, 4) and np.array_equal(g, RO.resample(x, taps, 3, 5))
    assert np.array_equal(out.trialdefinition, [[0, 180, -60], [180, 300, 0], [300, 481, 20]])
    assert out.samplerate == 600.0 and list(out.channel) == list(data.channel) and out.dimord == data.dimord
    assert out.data.dtype == np.float32 and "nan_trials" not in out.info
    assert out.cfg["earlier"] == {"a": 1}
    assert out.cfg["resampledata"] == dict(resamplefs=600, method="resample", lpfreq=None, order=None)

    long = _data(lengths=(1500, 1200), nchan=2)
    out = spy.resampledata(long, resamplefs=600, **HOW)                       # order 1000
    taps = design.windowed_sinc("hamming", 1000, 0.1) * 3
    assert np.array_equal(out.trials[1], RO.resample(long.trials[1], taps, 3, 5))
    with pytest.warns(UserWarning, match="order"):
        out = spy.resampledata(data, resamplefs=441, lpfreq=100, order=61, chan_per_worker=2, parallel=False, **HOW)
    taps = design.windowed_sinc("hamming", 62, 0.1 / 441) * 441
    assert np.array_equal(out.trials[2], RO.resample(data.trials[2], taps, 441, 1000))
    assert [len(t) for t in out.trials] == [133, 89, 133]                  # ceil(n * 441 / 1000)
    assert out.cfg["resampledata"]["lpfreq"] == 100 and out.cfg["resampledata"]["order"] == 61


@pytest.mark.parametrize("fs,new_fs,up,down", [(1000, 600, 3, 5), (1000, 333, 333, 1000), (1000, 441, 441, 1000),
                                               (1000, 999, 999, 1000), (1000, 750, 3, 4), (2000, 1200, 3, 5),
                                               (30000, 1000, 1, 30)])
def test_up_down_of_the_ratios(fs, new_fs, up, down):
    seen = {}

    def spy_resample(x, taps, u, d):
        seen["ud"] = (u, d, len(taps))
        return RO.resample(x, taps, u, d)
    data = _data(lengths=(120, 90), nchan=2, fs=float(fs))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = spy.resampledata(data, resamplefs=new_fs, compute_method="sequential",
                               routine_classes=dict(RO.RESAMPLE_OPS, resample=spy_resample))
    assert seen["ud"] == (up, down, 91)
    assert [len(t) for t in out.trials] == [-(-120 * up // down), -(-90 * up // down)]


def test_downsample_selection_and_unequal_lengths():
    data = _data(lengths=(300, 203, 300, 121), nchan=5)
    out = spy.resampledata(data, resamplefs=250, method="downsample", **HOW)
    for g, x in zip(out.trials, data.trials):
        assert np.array_equal(g, x[::4])
    assert np.array_equal(out.trialdefinition[:, :2], [[0, 75], [75, 126], [126, 201], [201, 232]])
    out = spy.resampledata(data, resamplefs=250, method="downsample", lpfreq=100, order=40, **HOW)
    taps = design.windowed_sinc("hamming", 40, 0.1)
    assert np.array_equal(out.trials[1], RO.PO.fir(RO.PO.fir(data.trials[1], taps), taps)[::4])
    sel = {"trials": [2, 1], "channel": [3, 1], "latency": [0.02, 0.15]}
    out = spy.resampledata(data, resamplefs=600, order=100, select=sel, **HOW)
    assert data.selection is None and list(out.channel) == list(data.channel[[3, 1]])
    taps = design.windowed_sinc("hamming", 100, 0.1) * 3
    assert np.array_equal(out.trials[0], RO.resample(data.trials[2][20:151][:, [3, 1]], taps, 3, 5))
    assert np.array_equal(out.trialdefinition, [[0, 79, 12], [79, 158, 12]])
    assert out.cfg["resampledata"]["select"] == sel


def test_warning_for_integer_ratio():
    with pytest.warns(UserWarning, match="downsample"):
        out = spy.resampledata(_data(), resamplefs=500, **HOW)
    assert [len(t) for t in out.trials] == [150, 100, 150]


@pytest.mark.parametrize("kw,exc", [
    (dict(method="decimate", resamplefs=500), SPYValueError), (dict(resamplefs=0.5), SPYValueError),
    (dict(resamplefs=1001), SPYValueError), (dict(resamplefs="fast"), SPYTypeError),
    (dict(resamplefs=600, order=-2), SPYValueError), (dict(resamplefs=600, order=100.5), SPYValueError),
    (dict(resamplefs=600, order="high"), SPYTypeError),
    (dict(resamplefs=600, lpfreq=301), SPYValueError), (dict(resamplefs=600, lpfreq=-1), SPYValueError),
    (dict(resamplefs=600, lpfreq=0), SPYValueError),
    (dict(resamplefs=600, method="downsample"), SPYValueError), (dict(resamplefs=600, foo=1), SPYValueError),
])
def test_argument_errors(kw, exc):
    with pytest.raises(exc):
        spy.resampledata(_data(), **kw, **HOW)


def test_input_errors():
    with pytest.raises(SPYTypeError):
        spy.resampledata(np.zeros((10, 2)), resamplefs=600, **HOW)
    with pytest.raises(SPYValueError):
        spy.resampledata(spy.AnalogData(), resamplefs=600, **HOW)


# ---- CPU emulation of resample_kernel.h ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    """the library's own launcher of csrc/resample.hip on the CPU, with a context of default launch limits"""
    lib = build_emu.emulated_library("resample")
    lib.emu_upfirdn_small.restype, lib.emu_upfirdn_small.argtypes = SIGNATURES["spyhip_upfirdn"]
    lib.ctx = build_emu.ctx(lib)
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


SMALL, LIBRARY = (2, 8, (4, 1)), (8, 128, (8, 4, 1))        # waves, taps per chunk, outputs per lane to choose from


def _run(emu, x, taps, up, down, nout=None, tiles=SMALL, ctx=None):
    """(result, outputs per lane of the tile that ran, trials per launch).  The tile is read from the launch log: the
    dynamic LDS of UpfirdnTile (csrc/resample_kernel.h) differs between the outputs per lane at one `down`."""
    T, N, Cn = x.shape
    nout = -(-N * up // down) if nout is None else nout
    out = np.full((T, nout, Cn), np.nan, dtype=np.float32)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    emu.emu_launch_log_reset()
    fn = emu.emu_upfirdn_small if tiles is SMALL else emu.spyhip_upfirdn
    assert fn(ctx or emu.ctx, _p(x), _p(out), T, N, Cn, nout, _p(taps), len(taps), up, down) == 0
    g = build_emu.launches(emu)
    nt, kc, choices = tiles
    lds = {r: max(((r - 1) * down + kc) * 64 * 4, nt * r * 64 * 8) for r in choices}
    assert len(set(lds.values())) == len(choices) and len(set(g[:, 6])) == 1 and np.all(g[:, 3] == 64 * nt)
    (r,) = [r for r in choices if lds[r] == g[0, 6]]
    return out, r, [int(z) for z in g[:, 2]]


def _batch(T, N, Cn, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(T, N, Cn)) + rng.normal(size=(T, 1, Cn))).astype(np.float32)


# the emulated tiles: 4 outputs per lane (1 when down > 8), 2 waves sharing chunks of 8 taps of a phase
SHAPES = [
    (3, 5, 40, 49),      # 16 or 17 taps per phase: two chunks and one tap of a third
    (3, 5, 20, 24),      # exactly one chunk per phase; 12 outputs = one block of 4 per phase
    (3, 5, 21, 25),      # 13 outputs: one past the block; 8 and 9 taps per phase
    (3, 5, 19, 23),      # 7 and 8 taps per phase
    (3, 4, 17, 31), (2, 3, 33, 15),
    (1, 8, 70, 17), (1, 9, 70, 17),      # the last `down` of the 4-output tile and the first of the 1-output tile
    (1, 30, 95, 41), (7, 3, 9, 29),
    (5, 7, 6, 61),       # taps far longer than the trial
    (40, 41, 12, 13),    # up > ntaps: phases without a tap
    (333, 1000, 50, 51), (3, 50, 30, 9),
]
# every shape at 65 channels; both tiles at and next to the 64-channel boundary
EMU_CASES = [s + (65,) for s in SHAPES] + [s + (c,) for s in (SHAPES[0], SHAPES[7]) for c in (1, 63, 64)]


@pytest.mark.parametrize("up,down,N,ntaps,nchan", EMU_CASES)
def test_emu_upfirdn(emu, up, down, N, ntaps, nchan):
    x = _batch(2, N, nchan, seed=up + down)
    taps = np.random.default_rng(ntaps).normal(size=ntaps)
    got, r, _ = _run(emu, x, taps, up, down)
    assert r == (4 if 3 * down + 8 <= 32 else 1)
    for t in range(2):
        ref = RO.resample64(x[t], taps, up, down)
        assert got[t].shape == ref.shape
        assert_parity(got[t], ref, what=f"upfirdn {up}/{down}")


def test_emu_three_trials_single_output_and_decimation(emu):
    x = _batch(3, 7, 5, seed=1)
    taps = np.random.default_rng(2).normal(size=11)
    got, _, _ = _run(emu, x, taps, 1, 7)                          # one output per trial
    assert got.shape == (3, 1, 5)
    for t in range(3):
        assert_parity(got[t], RO.resample64(x[t], taps, 1, 7), what="nout 1")
    x = _batch(3, 45, 65, seed=3)
    for skip in (1, 4, 8, 9, 44, 45, 100):
        got, _, _ = _run(emu, x, np.ones(1), 1, skip)
        assert np.array_equal(got, x[:, ::skip]), skip
    taps = design.windowed_sinc("hamming", 20, 0.1)            # the decimating second pass of downsample with lpfreq
    for skip in (4, 1):                                        # skip 1: a plain "same" filter (resample_poly copies there)
        got, _, _ = _run(emu, x, taps, 1, skip)
        for t in range(3):
            assert_parity(got[t], RO.PO.fir64(x[t], taps)[::skip], what="decimating same")


# the library's tiles: (R - 1) * down + 128 staged rows within 256 - the last `down` of 8 outputs per lane and the first of
# 4, the last of 4 and the first of 1; 129 taps are one chunk of 128 and one tap of a second at up = 1
@pytest.mark.parametrize("up", [1, 3])
@pytest.mark.parametrize("down,outputs", [(18, 8), (19, 4), (42, 4), (43, 1)])
def test_emu_upfirdn_library_tiles(emu, down, outputs, up):
    x = _batch(2, 70, 65, seed=up + down)
    taps = np.random.default_rng(129).normal(size=129)
    got, r, _ = _run(emu, x, taps, up, down, tiles=LIBRARY)
    assert r == outputs
    for t in range(2):
        # 3 / 18 and 3 / 42 share a factor, which resample_poly (RO.resample64) divides out before it filters: the
        # reference is its own upfirdn expression on the pair as given, which IS resample64 on the reduced pairs
        ref = RO.upfirdn64(x[t], taps, up, down)
        if np.gcd(up, down) == 1:
            same = RO.resample64(x[t], taps, up, down)          # (taps / up * up there: a rounding of the taps apart)
            assert np.abs(ref - same).max() <= 1e-14 * np.abs(same).max()
        assert got[t].shape == ref.shape
        assert_parity(got[t], ref, what=f"upfirdn {up}/{down}, library tile")


def test_emu_upfirdn_trial_chunks_and_refusal(emu):
    """7 trials at 3 per launch: the offsets of input and output in the loop over grid.z"""
    x = _batch(7, 70, 65, seed=11)
    taps = np.random.default_rng(12).normal(size=129)
    ref, _, z = _run(emu, x, taps, 3, 19, tiles=LIBRARY)
    assert z == [7]
    got, _, z = _run(emu, x, taps, 3, 19, tiles=LIBRARY, ctx=build_emu.ctx(emu, grid_yz=3))
    assert z == [3, 3, 1]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    for t in range(7):
        assert_parity(got[t], RO.resample64(x[t], taps, 3, 19), what="upfirdn in chunks of trials")
    assert emu.spyhip_upfirdn(emu.ctx, _p(x), _p(x), 7, 70, 65, 12, _p(taps), 129, 3, 19) == -1         # in == out
