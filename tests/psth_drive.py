"""What the CPU emulation (tests/test_psth.py) and the GPU tests (tests/test_gpu_psth.py) share: the recorded cases, the
inputs of the four kernels of csrc/psth_kernel.h from raw arrays or from a `_plan` of the front end, spike tables aimed
at the kernels' dispatch edges, and the emulator's driver."""
import ctypes as C
import os
import types

import numpy as np

import build_emu as BE
import psth_oracle as PO
import syncopy_amd as spy
from syncopy_amd.statistics import spike_psth as SP

HERE = os.path.dirname(os.path.abspath(__file__))
OUTPUTS = ("rate", "spikecount", "proportion")
# the tile extents of csrc/psth_kernel.h (test_psth.py checks them against the header through the emulator)
BIN_TILE, COL_TILE, UNIT_TILE, PROP_TILE, THREADS = 32, 128, 1024, 64, 256

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(HERE, "golden", "psth.npz")) as g:
            _golden = {k: g[k] for k in g.files}
    return _golden


def golden_names():
    return [str(n) for n in golden()["names"]]


def golden_case(name):
    g = golden()
    return g[f"{name}_spikes"], g[f"{name}_par"], g[f"{name}_edges"], g[f"{name}_columns"]


def inputs_from_columns(table, trl, edges, output, samplerate, columns):
    """kernel inputs for the trials `trl` (T, 3) [start, end, onset] and GIVEN columns (ncols, 2) - which may hold pairs
    that do not occur"""
    table = np.asarray(table, dtype=np.int64)
    trl = np.asarray(trl, dtype=np.float64).reshape(-1, 3)
    columns = np.asarray(columns, dtype=np.int64)
    nchan = int(max(table[:, 1].max(), columns[:, 0].max())) + 1
    nunit = int(max(table[:, 2].max(), columns[:, 1].max())) + 1
    flags = np.zeros((nchan, nunit), dtype=np.uint8)
    flags[columns[:, 0], columns[:, 1]] = 1
    cols, lut, unit_k, col_k, nk = SP.column_tables(flags)
    rows = np.searchsorted(table[:, 0], trl[:, :2].astype(np.int64).ravel()).reshape(-1, 2).astype(np.int64)
    lohi = np.array([SP.valid_bins(edges, s, e, o, samplerate) for s, e, o in trl], dtype=np.int32).reshape(-1, 2)
    return types.SimpleNamespace(
        edges=np.ascontiguousarray(edges, dtype=np.float64), nbins=len(edges) - 1, columns=cols, ncols=len(cols),
        lut=lut, C=nchan, U=nunit, unit_k=unit_k, col_k=col_k, nk=nk, row_lo=np.ascontiguousarray(rows[:, 0]),
        row_hi=np.ascontiguousarray(rows[:, 1]), start=trl[:, 0].astype(np.int64), onset=trl[:, 2].astype(np.int64),
        lohi=lohi, scale=float(1 / np.diff(edges)[0]) if output == "rate" else 1.0, output=output,
        samplerate=float(samplerate), trial_ids=list(range(len(trl))))


def oracle_for(data, plan, select=None):
    """the model's stacked result for a plan of the front end, and its columns"""
    sel = select or {}
    chans = None if sel.get("channel") is None else spy.datatype.SpikeSelection(data, {"channel": sel["channel"]}).channel
    units = None if sel.get("unit") is None else spy.datatype.SpikeSelection(data, {"unit": sel["unit"]}).unit
    return PO.psth(data.data, data.trialdefinition, plan.trial_ids, plan.edges, plan.output, data.samplerate, chans, units)


# ---- spike tables -------------------------------------------------------------------------------------------------
def make_data(trials, samplerate=1000.0, nchan=3, nunit=4, per_trial=60, seed=0, gap=50, between=0, first=0,
              pairs=None):
    """SpikeData of len(trials) trials given as (length, onset): `per_trial` random spikes each (an int, or one per
    trial), every pair of `pairs` (default: all nchan x nunit) drawn at random, `between` spikes in the gap behind
    every trial, the first trial starting at sample `first`"""
    rng = np.random.default_rng(seed)
    pairs = [(c, u) for c in range(nchan) for u in range(nunit)] if pairs is None else list(pairs)
    rows, trl, at = [], [], int(first)
    for k, (n, onset) in enumerate(trials):
        m = per_trial if np.isscalar(per_trial) else per_trial[k]
        s = np.sort(rng.integers(at, at + n, size=m))
        which = rng.integers(0, len(pairs), size=m)
        which[:min(m, len(pairs))] = rng.permutation(len(pairs))[:min(m, len(pairs))]
        rows += [(int(a), pairs[w][0], pairs[w][1]) for a, w in zip(s, which)]
        trl.append((at, at + n, onset))
        rows += [(int(a), pairs[0][0], pairs[0][1]) for a in rng.integers(at + n, at + n + gap, size=between)]
        at += n + gap
    return spy.SpikeData(np.array(rows, dtype=np.int64).reshape(-1, 3), samplerate=samplerate,
                         trialdefinition=np.array(trl, dtype=float))


def edge_adversary(samplerate, exact, start=3_000_000_000):
    """(data, window, binsize): one trial whose spikes sit at floor(e * sr) and ceil(e * sr) relative samples for every
    edge e of np.arange(w0, w1 + binsize, binsize): any deviation from IEEE division or from < / <= moves a count.
    exact=False: bins of 256 samples, so every edge lies within a few float64 ulp of a sample time.  exact=True: a
    window and bins of binary fractions whose last edge (and others) IS a sample time, with spikes on it.  The trial
    starts above 2^31."""
    if not exact:
        onset, binsize, nb = -3000, 256 / samplerate, 40
    elif samplerate == 30000.0:
        onset, binsize, nb = -3750, 1 / 64, 32                 # edges -0.125 + k / 64; every fourth is a sample time
    else:
        assert samplerate == 24414.0625
        onset, binsize, nb = 0, 0.25, 64                       # 16 s = 390625 samples
    w0 = onset / samplerate
    w1 = w0 + nb * binsize
    edges = np.arange(w0, w1 + binsize, binsize)
    last = int(np.rint(edges[-1] * samplerate))
    assert not exact or last / samplerate == edges[-1]
    rel = np.concatenate([np.floor(edges * samplerate), np.ceil(edges * samplerate), [last, last, last - 1, last + 1]])
    rel = np.sort(rel.astype(np.int64) - onset)
    n = last - onset + 500
    rel = rel[(rel >= 0) & (rel < n)]
    tab = np.stack([start + rel, np.arange(rel.size) % 2, np.arange(rel.size) % 3], axis=1)
    data = spy.SpikeData(tab, samplerate=samplerate, trialdefinition=[[start, start + n, onset]])
    return data, [w0, w1], binsize


# ---- the emulator --------------------------------------------------------------------------------------------------
def build_emu():
    """the library's own launchers of csrc/psth.hip on the CPU, with a context of default launch limits"""
    lib = BE.emulated_library("psth")
    lib.emu_psth_tiles.argtypes = [C.c_void_p] * 5
    lib.ctx = BE.ctx(lib)
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _columns(table):
    table = np.asarray(table, dtype=np.int64)
    return (np.ascontiguousarray(table[:, 0]), np.ascontiguousarray(table[:, 1], dtype=np.int32),
            np.ascontiguousarray(table[:, 2], dtype=np.int32))


def emu_presence(lib, table):
    """the `presence` argument of _plan through the emulated psth_presence_kernel"""
    _, chan, unit = _columns(table)

    def presence(pre):
        flags = np.zeros(pre.C * pre.U, dtype=np.uint8)
        assert lib.spyhip_psth_presence(lib.ctx, _p(chan), _p(unit), _p(pre.row_lo), _p(pre.row_hi), len(pre.row_lo),
                                        int((pre.row_hi - pre.row_lo).max()), _p(pre.chan_ok), pre.C, _p(pre.unit_ok),
                                        pre.U, _p(flags)) == 0
        return flags
    return presence


def emu_histogram(lib, table, k):
    """the stacked (T * nbins, ncols) float32 result of the emulated kernels for kernel inputs `k` (a _plan of the front
    end, or inputs_from_columns); the buffers start out poisoned"""
    sample, chan, unit = _columns(table)
    T = len(k.row_lo)
    rows = np.full((T, k.nbins + 1), -(1 << 40), dtype=np.int64)
    assert lib.spyhip_psth_bin_rows(lib.ctx, _p(sample), _p(k.row_lo), _p(k.row_hi), _p(k.start), _p(k.onset), T,
                                    _p(k.edges), k.nbins + 1, k.samplerate, _p(rows)) == 0
    assert np.all(rows >= k.row_lo[:, None]) and np.all(rows <= k.row_hi[:, None]) and np.all(np.diff(rows, axis=1) >= 0)
    out = np.full((T, k.nbins, k.ncols), -7.0, dtype=np.float32)
    lib.emu_launch_log_reset()
    assert lib.spyhip_psth_count(lib.ctx, _p(chan), _p(unit), _p(rows), _p(k.lut), k.C, k.U, _p(k.lohi), T, k.nbins,
                                 k.ncols, k.scale, _p(out)) == 0
    (grid,) = BE.launches(lib)[:, :3]
    assert grid.prod() == T * -(-k.nbins // BIN_TILE) * -(-k.ncols // COL_TILE)
    if k.output == "proportion":
        S = np.full((T, k.nk), -9, dtype=np.int32)
        assert lib.spyhip_psth_proportion(lib.ctx, _p(chan), _p(unit), _p(k.row_lo), _p(k.row_hi), _p(rows), _p(k.lut),
                                          k.C, k.U, _p(k.unit_k), _p(k.col_k), k.nk, _p(k.edges), T, k.nbins, k.ncols,
                                          _p(S), _p(out)) == 0
        assert np.all(S >= -1)
    return out.reshape(T * k.nbins, k.ncols)
