"""NumPy model of spy.selectdata for the tests: per selected trial `data[a:b][np.ix_(...)]`, stacked, with the
trialdefinition and the labels the result must carry.  Written from the reference's rules (datatype/selector.py,
shared/latency.py, shared/tools.py: best_match), not from the front end's planner."""
import numpy as np

_LABELS = {"channel": "channel", "channel_i": "channel_i", "channel_j": "channel_j", "taper": "taper", "freq": "frequency"}


def gather(data, trials, axes=None):
    """rows [a, b) of `data` per trial, of every row the entries that `axes` names (per inner axis None, (start, count) or
    an index array), stacked"""
    data = np.asarray(data)
    axes = [None] * (data.ndim - 1) if axes is None else axes
    inner = []
    for spec, extent in zip(axes, data.shape[1:]):
        if spec is None:
            inner.append(np.arange(extent))
        elif isinstance(spec, tuple):
            inner.append(np.arange(spec[0], spec[0] + spec[1]))
        else:
            inner.append(np.asarray(spec, dtype=np.int64))
    parts = [data[a:b][np.ix_(np.arange(b - a), *inner)] for a, b in trials]
    shape = (0,) + tuple(len(i) for i in inner)
    return np.concatenate(parts, axis=0) if parts else np.empty(shape, dtype=data.dtype)


def _indices(spec, labels, extent):
    if spec is None:
        return np.arange(extent)
    if isinstance(spec, slice):
        return np.arange(extent)[spec]
    names = None if labels is None else [str(s) for s in labels]
    return np.array([names.index(c) if isinstance(c, str) else int(c) for c in (spec if np.ndim(spec) else [spec])],
                    dtype=np.int64)


def _frequency(spec, freq):
    freq = np.asarray(freq, dtype=float)
    if spec is None:
        return np.arange(freq.size)
    if np.ndim(spec) == 0:
        return np.array([int(np.argmin(np.abs(freq - spec)))])          # (the tests pick no tie)
    return np.nonzero((freq >= spec[0]) & (freq <= spec[1]))[0]


def selectdata(obj, trials=None, latency=None, **keys):
    """(data, trialdefinition, labels): what spy.selectdata(obj, ...) must hold; latency: [t0, t1] in seconds or None"""
    trl = np.asarray(obj.trialdefinition, dtype=float)
    ids = list(range(trl.shape[0])) if trials is None else [int(t) for t in trials]
    windows = {}
    for t in set(ids):
        n = int(trl[t, 1] - trl[t, 0])
        time = (np.arange(n) + trl[t, 2]) / obj.samplerate
        if latency is None:
            windows[t] = (0, n)
        elif n and time[0] <= latency[0] and time[-1] >= latency[1]:     # the trial covers the window
            inside = np.nonzero((time >= latency[0]) & (time <= latency[1]))[0]
            windows[t] = (int(inside[0]), int(inside[-1]) + 1) if inside.size else (0, 0)
    ids = [t for t in ids if t in windows]                                # the others are discarded
    inner, labels = [], {}
    for dim, extent in zip(obj.dimord[1:], obj.data.shape[1:]):
        have = getattr(obj, dim, None)
        spec = keys.get(_LABELS[dim])
        idx = _frequency(spec, have) if dim == "freq" else _indices(spec, have, extent)
        inner.append(idx)
        labels[dim] = None if have is None else np.asarray(have)[idx]
    rows = [(int(trl[t, 0]) + windows[t][0], int(trl[t, 0]) + windows[t][1]) for t in ids]
    data = gather(obj.data, rows, inner)
    new, at = np.zeros((len(ids), trl.shape[1])), 0
    for k, t in enumerate(ids):
        a, b = windows[t]
        new[k, :3] = [at, at + (b - a), a + trl[t, 2] if b > a else 0]
        new[k, 3:] = trl[t, 3:]
        at += b - a
    return data, new, labels
