"""`spy.selectdata` and `spy.copy`: a new data object that holds the selected trials, time window, channels, frequencies
and tapers of another (syncopy/datatype/methods/selectdata.py:256-423, datatype/selector.py, methods/copy.py), gathered on
the device (csrc/select.hip), in one launch from a device copy or one per chunk of uploaded trials.

Every value is moved as raw bits: the result is what `data[a:b][np.ix_(...)]` gives per selected trial, stacked in
selection order.  `_plan` is everything above the kernel (NumPy only: checks, index lists, the per-trial row table, the
result's shape and labels), `_run` the device part.  There is no CPU path.

Deviations from the reference, on purpose:
  * `inplace=True` takes `trials`, `channel` and `latency` only (what `datatype.Selection` holds); the other keys need a
    deep copy and say so;
  * the input's own `.selection` is left as it was found (the reference overwrites it with the keywords and then wipes it);
    as in the reference the keywords alone decide what is selected;
  * SpikeData is refused; the data must be float32, float64, complex64 or complex128.
"""
import types

import numpy as np

from ..shared.errors import SPYInfo, SPYTypeError, SPYValueError
from ..shared.latency import create_trial_selection, get_analysis_window
from ..shared.tools import best_match

__all__ = ["selectdata", "copy"]

# bytes of host trials that are on the device at once when the source has no device copy
CHUNK_BYTES = 512 << 20

# the kinds of an axis of spyhip_select (include/spyhip.h)
WHOLE, RANGE, LIST = 0, 1, 2

_SELECTORS = ("trials", "channel", "channel_i", "channel_j", "latency", "frequency", "taper")
_INPLACE_KEYS = ("trials", "channel", "latency")
# the selector of an inner dimension and the property that labels it
_DIM_KEY = {"channel": "channel", "channel_i": "channel_i", "channel_j": "channel_j", "freq": "frequency", "taper": "taper"}


def _selection_keywords(data):
    from . import AnalogData, CrossSpectralData, SpectralData, TimeLockData
    if isinstance(data, (AnalogData, TimeLockData)):
        return ("trials", "channel", "latency")
    if isinstance(data, SpectralData):
        return ("trials", "channel", "latency", "frequency", "taper")
    if isinstance(data, CrossSpectralData):
        return ("trials", "channel_i", "channel_j", "latency", "frequency")
    raise SPYTypeError(data, varname="data", expected="`AnalogData`, `TimeLockData`, `SpectralData` or `CrossSpectralData`")


def select_axes(inner, axes):
    """(extent, kind, start, count, idx) of spyhip_select for a row of shape `inner` (up to three axes; missing ones are
    added in front with extent 1): per axis None (all of it), (start, count) or an array of indices; idx: the index arrays
    one after the other (int32), or None"""
    inner = tuple(int(s) for s in inner)
    axes = [None] * len(inner) if axes is None else list(axes)
    assert len(inner) <= 3 and len(axes) == len(inner)
    pad = 3 - len(inner)
    extent = np.array((1,) * pad + inner, dtype=np.int64)
    kind, start, count, lists = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int64), extent.copy(), []
    for i, spec in enumerate(axes, pad):
        if spec is None:
            continue
        if isinstance(spec, tuple):
            kind[i], start[i], count[i] = RANGE, int(spec[0]), int(spec[1])
        else:
            lists.append(np.ascontiguousarray(spec, dtype=np.int32).reshape(-1))
            kind[i], count[i] = LIST, lists[-1].size
    return extent, kind, start, count, (np.concatenate(lists) if lists else None)


# ---- the selectors (NumPy only) --------------------------------------------------------------------------------------------
def _resolve_labels(spec, labels, extent, key):
    """indices of a `channel`-like selector (indices, names, slice or range), or None for all of them"""
    if spec is None or (isinstance(spec, str) and spec == "all"):
        return None
    if isinstance(spec, slice):
        return list(range(extent))[spec]
    names = [] if labels is None else [str(s) for s in labels]
    idx = []
    for c in (spec if isinstance(spec, (list, tuple, range, np.ndarray)) else [spec]):
        if isinstance(c, (str, np.str_)):
            if str(c) not in names:
                raise SPYValueError(f"existing {key} names", varname=f"select: {key}", actual=str(c))
            idx.append(names.index(str(c)))
        elif isinstance(c, (bool, np.bool_)) or not np.issubdtype(type(c), np.integer):
            raise SPYValueError(f"{key} indices or names", varname=f"select: {key}", actual=str(c))
        else:
            idx.append(int(c))
    if any(c < 0 or c >= extent for c in idx):
        raise SPYValueError(f"{key} indices in [0, {extent})", varname=f"select: {key}", actual=str(spec))
    return idx


def _resolve_frequency(data, spec):
    """a scalar picks the closest bin, [fmin, fmax] every bin inside (selector.py:486-542, continuous_data.py:617-639)"""
    if spec is None or (isinstance(spec, str) and spec == "all"):
        return None
    if isinstance(spec, str):
        raise SPYValueError("'all' or `None` or float or list/array", varname="frequency", actual=spec)
    if getattr(data, "freq", None) is None:
        raise SPYValueError("Syncopy data object with freq-dimension", varname="frequency", actual=data.__class__.__name__)
    freq = np.asarray(data.freq, dtype=float)
    scalar = np.issubdtype(type(spec), np.number)
    try:
        lim = np.array([spec] if scalar else spec, dtype=float)
    except (TypeError, ValueError):
        lim = np.empty(0)
    if lim.shape != ((1,) if scalar else (2,)) or not np.isfinite(lim).all():
        raise SPYValueError("float or [fmin, fmax]", varname="frequency", actual=str(spec))
    if lim.min() < freq.min() or lim.max() > freq.max():
        raise SPYValueError(f"all array elements to be bounded by {freq.min()} and {freq.max()}", varname="frequency",
                            actual=str(spec))
    if scalar:
        return [int(i) for i in best_match(freq, lim)[1]]
    if lim[0] >= lim[1]:
        raise SPYValueError("`select: frequency` selection with `frequency[0]` < `frequency[1]`", varname="frequency",
                            actual=f"selection range from {lim[0]} to {lim[1]}")
    return [int(i) for i in best_match(freq, lim, span=True)[1]]


def _axis_spec(idx, extent):
    """None (the whole axis), (start, count) or an int32 index array: what the kernel is told about one axis"""
    if idx is None or list(idx) == list(range(extent)):
        return None
    if all(b - a == 1 for a, b in zip(idx[:-1], idx[1:])):
        return (int(idx[0]), len(idx))
    return np.array(idx, dtype=np.int32)


def _is_empty(obj):
    return (obj._data is None and obj._pending is None) or obj.trialdefinition is None


class _Trials:
    """What `Selection` and the latency functions read of a data object, without its channels: the trial selection is
    worked out on this stand-in, so the object's own `.selection` is never touched.  `time[t]` is the time axis of trial
    t as `_Base.time` computes it, made when a latency window asks for it."""

    def __init__(self, data):
        self.trialdefinition, self.sampleinfo, self.samplerate = data.trialdefinition, data.sampleinfo, data.samplerate
        self.trialintervals = data.trialintervals
        self.channel, self.selection, self.time = [], None, self

    def __getitem__(self, t):
        a, b = self.sampleinfo[t]
        return (np.arange(0, int(b - a)) + self.trialdefinition[t, 2]) / self.samplerate


def _trial_selection(data, trials, latency):
    """(stand-in, select): the `select` dictionary of the trials and the time window; the trials that do not cover a
    latency window are discarded first (selectdata.py:326-354)"""
    from . import Selection
    view = _Trials(data)
    select = {"trials": trials}
    if latency is not None and not (isinstance(latency, str) and latency == "all"):
        view.selection = Selection(view, select)
        window = get_analysis_window(view, latency)
        select, discarded = create_trial_selection(view, window)
        if discarded > 0:
            SPYInfo(f"Discarded {discarded} trial(s) which did not fit into latency window")
        select["latency"] = window
        view.selection = None
    return view, select


def _check_keys(data, keys, given):
    """every selector present (None: not given), and none that the class does not have (selectdata.py:304-309)"""
    for key in _SELECTORS:
        given.setdefault(key, None)
        if key not in keys and given[key] is not None:
            raise SPYValueError(f"one of {keys}", "selection arguments",
                                f"no `{key}` selection available for {data.__class__.__name__}")


def _plan(data, **given):
    from . import Selection
    from .arithmetic import _checked_dtype
    keys = _selection_keywords(data)
    if _is_empty(data):
        raise SPYValueError("non-empty Syncopy data object", varname="data", actual="empty object")
    _check_keys(data, keys, given)
    dimord = list(data.dimord)
    if dimord.index("time") != 0 or len(dimord) > 4:
        raise SPYValueError("data with time as its first dimension", varname="data", actual=f"dimord {dimord}")
    dtype = _checked_dtype(data.data_dtype, data.data_dtype, "data")
    full = tuple(int(s) for s in data.data_shape[1:])
    picked, axes = {}, []
    for dim, extent in zip(dimord[1:], full):
        key = _DIM_KEY[dim]
        if key == "frequency":
            idx = _resolve_frequency(data, given[key])
        else:
            idx = _resolve_labels(given[key], getattr(data, dim, None), extent, key)
        if idx is not None and len(idx) == 0:
            raise SPYValueError(f"at least one selected {key}", varname=f"select: {key}", actual=str(given[key]))
        picked[dim] = idx
        axes.append(_axis_spec(idx, extent))
    sel = Selection(*_trial_selection(data, given["trials"], given["latency"]))
    si = data.sampleinfo
    rows = [(int(si[t, 0] + sel.time[t][0]), int(si[t, 0] + sel.time[t][1])) for t in sel.trial_ids]
    if any(a < 0 or b > data.data_shape[0] or b < a for a, b in rows):
        raise SPYValueError("trials inside the data", varname="trialdefinition", actual=f"rows {rows}")
    starts = np.concatenate(([0], np.cumsum([b - a for a, b in rows]))).astype(np.int64)
    inner = tuple(extent if idx is None else len(idx) for idx, extent in zip((picked[d] for d in dimord[1:]), full))
    log = {key: given[key] for key in keys}
    log.update(inplace=False, clear=False)
    return types.SimpleNamespace(base=data, dtype=dtype, rows=rows, axes=axes, picked=picked, full=full, inner=inner,
                                 starts=starts[:-1], nrows=int(starts[-1]), trialdefinition=sel.trialdefinition.copy(),
                                 trial_ids=list(sel.trial_ids), log=log)


def _new_object(plan):
    """the result object without its data: class, dimord, trials and the labels in selection order"""
    base = plan.base
    out = base.__class__(None, samplerate=base.samplerate, dimord=base.dimord)
    out.trialdefinition = plan.trialdefinition
    for prop in ("freq", "taper", "channel", "channel_i", "channel_j"):
        if getattr(base, prop, None) is not None:
            labels, idx = np.array(getattr(base, prop)), plan.picked.get(prop)
            setattr(out, prop, labels if idx is None or prop not in base.dimord else labels[idx])
    out.cfg = dict(base.cfg)
    out.cfg["selectdata"] = dict(plan.log)
    return out


# ---- the device part ------------------------------------------------------------------------------------------------------
def _adopt(out, res, dtype):
    """`res` becomes the data of `out` and stays on the device"""
    from . import AnalogData, CrossSpectralData
    from .. import backend
    if isinstance(out, AnalogData) and dtype in (np.float32, np.complex64):
        out.adopt_device_result(res)
        return
    out.set_pending(lambda: backend.to_host(res), res.shape, dtype)
    if isinstance(out, CrossSpectralData):
        out._dev = res
    else:
        out._resident = res


def _run(plan, out):
    import torch
    from .arithmetic import _host_chunks, _resident
    from .. import backend
    backend.require_gpu()
    base = plan.base
    dev, origin = _resident(base)
    device = dev.device if dev is not None else torch.device("cuda", torch.cuda.current_device())
    tdtype = torch.from_numpy(np.empty(0, dtype=plan.dtype)).dtype
    res = torch.empty((plan.nrows,) + plan.inner, dtype=tdtype, device=device)
    n = np.array([b - a for a, b in plan.rows], dtype=np.int64)
    if dev is not None:                                           # read where it lies
        a0 = np.array([a - origin for a, _ in plan.rows], dtype=np.int64)
        backend.select(dev, np.stack([plan.starts, a0, n], axis=1), res, plan.axes)
    else:                                                         # the selected rows with all inner axes, chunk by chunk
        host = base.data
        src = types.SimpleNamespace(base=base, rows=plan.rows, inner=plan.full)
        for k0, k1 in _host_chunks(src, CHUNK_BYTES):
            local = np.concatenate(([0], np.cumsum(n[k0:k1])))
            if local[-1] == 0:
                continue
            stage = torch.empty((int(local[-1]),) + plan.full, dtype=tdtype, device=device)
            for k in range(k0, k1):
                a, b = plan.rows[k]
                if b > a:
                    stage[int(local[k - k0]):int(local[k - k0 + 1])].copy_(torch.from_numpy(np.ascontiguousarray(host[a:b])))
            backend.select(stage, np.stack([plan.starts[k0:k1], local[:-1], n[k0:k1]], axis=1), res, plan.axes)
    _adopt(out, res, plan.dtype)


# ---- the front ends ---------------------------------------------------------------------------------------------------------
def selectdata(data, trials=None, channel=None, channel_i=None, channel_j=None, latency=None, frequency=None, taper=None,
               inplace=False, clear=False, **kwargs):
    """A new object of `data`'s class that holds the selected part of it (`inplace=False`), or an in-place selection on
    `data` itself (`inplace=True`: `trials`, `channel` and `latency` only; returns None).  `clear=True` removes an in-place
    selection.

    trials: indices, any order, repeats allowed; channel / channel_i / channel_j / taper: indices, names, slice or range;
    latency: [t0, t1] in seconds or 'maxperiod', 'minperiod', 'prestim', 'poststim' (trials that do not cover the window
    are discarded); frequency: a scalar (the closest bin) or [fmin, fmax]."""
    from . import Selection, SpikeData, _Base
    if not isinstance(data, _Base) or isinstance(data, SpikeData):
        raise SPYTypeError(data, varname="data", expected="`AnalogData`, `TimeLockData`, `SpectralData` or `CrossSpectralData`")
    if not isinstance(inplace, bool):
        raise SPYTypeError(inplace, varname="inplace", expected="Boolean")
    if not isinstance(clear, bool):
        raise SPYTypeError(clear, varname="clear", expected="Boolean")
    if "select" in kwargs:
        raise SPYValueError("unpacked selection keywords directly, try `**select`", varname="selection kwargs",
                            actual="`select` as explicit parameter")
    keys = _selection_keywords(data)
    if kwargs:
        raise SPYValueError(f"the following keywords for {data.__class__.__name__}: {keys} and 'inplace', 'clear'",
                            varname="selection kwargs", actual=f"dict with keys {sorted(kwargs)}")
    given = {"trials": trials, "channel": channel, "channel_i": channel_i, "channel_j": channel_j, "latency": latency,
             "frequency": frequency, "taper": taper}
    _check_keys(data, keys, given)
    if clear:
        if any(value is not None for value in given.values()):
            raise SPYValueError("no data selectors if `clear = True`", varname="select",
                                actual={k: v for k, v in given.items() if v is not None})
        data.selection = None
        return None
    log = {key: given[key] for key in keys}
    log.update(inplace=inplace, clear=clear)
    if inplace:
        deep = [key for key in keys if key not in _INPLACE_KEYS and given[key] is not None]
        if deep:
            raise SPYValueError("`trials`, `channel` or `latency` with `inplace=True`: a deep copy is needed "
                                "(`inplace=False`) to select " + ", ".join(f"`{k}`" for k in deep),
                                varname="inplace", actual=f"in-place selection of {deep}")
        if _is_empty(data):
            raise SPYValueError("non-empty Syncopy data object", varname="data", actual="empty object")
        _, select = _trial_selection(data, trials, latency)
        if channel is not None:
            select["channel"] = channel
        data.selection = Selection(data, {k: v for k, v in select.items() if v is not None})
        data.cfg.update({"selectdata": log})
        return None
    plan = _plan(data, **given)
    out = _new_object(plan)
    _run(plan, out)
    return out


def copy(data):
    """A deep copy of `data` with every label and its cfg; made on the device where the data lies there (the selection
    kernel with everything taken whole), else on the host."""
    from . import SpikeData, TimeLockData, _Base
    from .arithmetic import DTYPES, _resident
    if not isinstance(data, _Base) or isinstance(data, SpikeData):
        raise SPYTypeError(data, varname="data", expected="`AnalogData`, `TimeLockData`, `SpectralData` or `CrossSpectralData`")
    out = data.__class__(None, samplerate=data.samplerate, dimord=data.dimord)
    if data.trialdefinition is not None:
        out.trialdefinition = data.trialdefinition.copy()
    for prop in ("freq", "taper", "channel", "channel_i", "channel_j") + (("avg", "var", "cov") if isinstance(data, TimeLockData) else ()):
        if getattr(data, prop, None) is not None:
            setattr(out, prop, np.array(getattr(data, prop)))
    out.cfg, out.info, out.log = dict(data.cfg), dict(data.info), data.log
    if data._data is None and data._pending is None:
        return out
    dev, origin = (None, 0) if np.dtype(data.data_dtype) not in DTYPES or len(data.data_shape) > 4 else _resident(data)
    if dev is None or origin != 0 or dev.shape[0] == 0:
        out.data = np.array(data.data)
        return out
    import torch
    from .. import backend
    res = torch.empty_like(dev)
    backend.select(dev, np.array([[0, 0, dev.shape[0]]], dtype=np.int64), res, None)
    _adopt(out, res, np.dtype(data.data_dtype))
    return out
