"""`spy.redefinetrial`: a copy of a data object with other trials - a subset, a time window, a minimum length, or new
sample ranges and offsets (syncopy/datatype/methods/redefinetrial.py:88-254, followed step by step).  The data moves
through `spy.selectdata` / `spy.copy`, on the device; what is edited here is the copy's trialdefinition."""
from numbers import Number

import numpy as np

from ..shared.errors import SPYError, SPYInfo, SPYTypeError, SPYValueError
from .selectdata import copy, selectdata

__all__ = ["redefinetrial"]


def redefinetrial(data, trials=None, minlength=None, offset=None, toilim=None, begsample=None, endsample=None, trl=None):
    """trials: indices of the trials to keep; minlength: seconds a trial must have; toilim: [t0, t1] in seconds, the
    window every kept trial is cut to; begsample / endsample: new first and one-past-last sample relative to each trial's
    start (scalars or one per trial); trl: a whole new trialdefinition; offset: new trigger offsets in samples (scalar or
    one per trial).  `minlength`, `toilim`, `begsample`/`endsample` and `trl` exclude each other."""
    from . import SpikeData, _Base
    if not isinstance(data, _Base) or isinstance(data, SpikeData):
        raise SPYTypeError(data, varname="data", expected="`AnalogData`, `TimeLockData`, `SpectralData` or `CrossSpectralData`")
    if (data._data is None and data._pending is None) or data.trialdefinition is None:
        raise SPYValueError("non-empty Syncopy data object", varname="data", actual="empty object")
    new_cfg = {"trials": trials, "minlength": minlength, "offset": offset, "toilim": toilim, "begsample": begsample,
               "endsample": endsample, "trl": trl}

    # -- mutually exclusive parameters
    if [minlength, toilim, begsample, trl].count(None) < 3:
        raise SPYError("Incompatible input arguments, either `minlength` or `begsample`/`endsample` or `trl` or `toilim`")
    scount = int(data.data_shape[0])                    # total number of samples

    # -- first select trials; a copy in any case
    if trials is not None:
        tr = np.asarray(trials)
        if tr.ndim != 1 or tr.dtype.kind not in "iu":
            raise SPYValueError("1-dimensional array of integers", varname="trials", actual=str(trials))
        ret = selectdata(data, trials=trials)
    else:
        ret = copy(data)

    # -- apply latency window
    if toilim is not None:
        lim = np.asarray(toilim)
        if lim.shape != (2,) or lim.dtype.kind not in "iuf":
            raise SPYValueError("[start, end] in seconds", varname="toilim", actual=str(toilim))
        ret = selectdata(ret, latency=toilim)
    elif minlength is not None:
        if isinstance(minlength, bool) or not isinstance(minlength, Number) or not 0 <= minlength < np.inf:
            raise SPYValueError("value to be greater or equals 0 and finite", varname="minlength", actual=str(minlength))
        min_samples = int(minlength * data.samplerate)
        si = ret.sampleinfo
        keep = [k for k in range(si.shape[0]) if si[k, 1] - si[k, 0] >= min_samples]
        SPYInfo(f"discarding {si.shape[0] - len(keep)} trials", caller="redefinetrial")
        if len(keep) == 0:
            SPYInfo("No trial fits the desired `minlength`, returning empty object!", caller="redefinetrial")
            return data.__class__()
        ret = selectdata(ret, trials=keep)
    new_trldef = ret.trialdefinition.copy()

    # -- OR manipulate sampleinfo
    if trl is not None:
        if [begsample, endsample, offset].count(None) < 3:
            raise SPYError("Incompatible input arguments, either complete trialdefinition `trl` or  "
                           "`begsample`/`endsample` and `offset`")
        try:
            trl = np.array(trl, dtype=float)
        except (TypeError, ValueError):
            raise SPYTypeError(trl, "trl", "array of numbers")
        if trl.ndim == 1:
            trl = trl[None, :]
        if trl.ndim != 2:
            raise SPYValueError("2-dimensional array", "trl", f"{trl.ndim} array")
        new_trldef = trl
    elif begsample is not None or endsample is not None:
        if begsample is None or endsample is None:
            raise SPYValueError("both `begsample` and `endsample`", "begsample/endsample", f"got [{begsample}, {endsample}]")
        try:
            begsample = np.array(begsample, dtype=int)
        except (TypeError, ValueError):
            raise SPYTypeError(begsample, "begsample", "integer number or array")
        try:
            endsample = np.array(endsample, dtype=int)
        except (TypeError, ValueError):
            raise SPYTypeError(endsample, "endsample", "scalar or array")
        if np.any(begsample < 0):
            raise SPYValueError("integers >= 0", "begsample", "relative `begsample` < 0")
        if begsample.size != 1 and begsample.size != len(new_trldef):
            raise SPYValueError(f"scalar or array of length {len(new_trldef)}", "begsample/endsample", "wrong sized `begsample`")
        if begsample.size != endsample.size:
            raise SPYValueError("same sizes for `begsample/endsample`", "", "different sizes")
        if np.any(new_trldef[:, 0] + endsample > scount):
            raise SPYValueError(f"integers < {int(scount - new_trldef[:, 0].max())}", "endsample", "out of range")
        if np.any(endsample - begsample < 0):           # this also catches negative endsample
            raise SPYValueError("endsample > begsample", "begsample/endsample", "endsample < begsample")
        new_trldef[:, 1] = new_trldef[:, 0] + endsample
        new_trldef[:, 0] += begsample

    # -- manipulate offset
    if isinstance(offset, Number) and not isinstance(offset, bool):
        new_trldef[:, 2] = np.ones(len(new_trldef)) * offset
    elif isinstance(offset, np.ndarray):
        if len(offset) != len(new_trldef):
            raise SPYValueError(f"array of length {len(new_trldef)}", "offset", f"array of length {len(offset)}")
        new_trldef[:, 2] = offset
    elif offset is not None:
        raise SPYTypeError(offset, "offset", "scalar, array or None")

    # -- apply the new trialdefinition: whole samples inside the copy's data
    if new_trldef.ndim != 2 or new_trldef.shape[1] < 3:
        raise SPYValueError("M x 3 array [start, stop, offset]", varname="trl", actual=f"{new_trldef.shape}")
    rows = new_trldef[:, :2]
    if not np.isfinite(rows).all() or np.any(rows != np.round(rows)) or np.any(rows < 0) or np.any(rows > scount):
        raise SPYValueError(f"integer samples bounded by 0 and {scount}", varname="trl", actual=str(rows.tolist()))
    # beyond the reference, whose limit is the input's sample count alone: after `trials=` or `toilim=` the copy holds
    # fewer rows than the input, and a trial must lie inside the rows that are there
    if np.any(rows[:, 1] > ret.data_shape[0]) or np.any(rows[:, 1] < rows[:, 0]):
        raise SPYValueError(f"trials inside the {ret.data_shape[0]} samples of the result", varname="trl",
                            actual=str(rows.tolist()))
    ret.trialdefinition = new_trldef
    ret.cfg.update(data.cfg)
    ret.cfg.update({"redefinetrial": new_cfg})
    return ret
