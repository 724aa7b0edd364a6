"""`spy.concat`: a new data object that holds the channels of two to eight others side by side, trial by trial
(syncopy/datatype/methods/concat.py: concat, concat_cF), joined on the device (csrc/concat.hip): one launch when every
source has a device copy, else one per chunk of uploaded trials.

Every value is moved as raw bits: trial k of the result is `np.concatenate([trial k of every object], axis=channel)`, and
the trials are stacked.  `_plan` is everything above the kernel (NumPy only: checks, the per-trial row table, labels),
`_run` the device part.  There is no CPU path.

Beyond the reference: more than two objects (up to 8) in one call.  Deviations from it, on purpose:
  * time must be the first dimension;
  * all objects must have one dtype, float32, float64, complex64 or complex128: the reference casts the second object to
    the first's dtype when it writes, here a mismatch is refused (the operators can cast);
  * an object with an active in-place selection is refused: the reference mixes the selected trials with the unselected
    channel counts.  `spy.selectdata(obj, ...)` makes the selection an object of its own first;
  * the channel labels are the sources' labels one after the other where they are all distinct (the reference always ends
    up with default labels); `avg` / `var` / `cov` of TimeLockData are not carried over.
"""
import types

import numpy as np

from ..shared.errors import SPYTypeError, SPYValueError

__all__ = ["concat"]

# bytes of host trials (of all sources without a device copy together) that are on the device at once
CHUNK_BYTES = 512 << 20

# SPYHIP_CONCAT_MAX of include/spyhip.h
MAX_OBJECTS = 8


def _default_labels(cls, nchan):
    """what the class's constructor gives `nchan` channels without names"""
    from . import AnalogData
    if cls is AnalogData:
        return np.array(["channel" + str(i + 1).zfill(len(str(nchan))) for i in range(nchan)])
    return None


def _plan(objs, dim="channel"):
    from . import AnalogData, CrossSpectralData, SpectralData, TimeLockData
    from .arithmetic import DTYPES
    from .selectdata import _is_empty
    first = objs[0]
    for i, obj in enumerate(objs):
        if not isinstance(obj, (AnalogData, SpectralData, CrossSpectralData, TimeLockData)):
            raise SPYTypeError(obj, f"spy_obj{i + 1}", "continuous data type")
    for i, obj in enumerate(objs):
        if _is_empty(obj):
            raise SPYValueError("non-empty Syncopy data object", varname=f"spy_obj{i + 1}", actual="empty object")
    for obj in objs[1:]:
        if obj.__class__ is not first.__class__ or list(obj.dimord) != list(first.dimord):
            raise SPYValueError("objects with equal dimensional layout", "spy object dimensions",
                                f"{first.__class__.__name__} {first.dimord} and {obj.__class__.__name__} {obj.dimord}")
    dimord = list(first.dimord)
    if dim not in dimord:
        raise SPYValueError(f"object which has a `{dim}` dimension", "spy_obj1.dimord", f"{dimord}")
    if dim != "channel":
        raise NotImplementedError("Only `channel` concatenation supported atm")
    axis = dimord.index(dim)
    shape = tuple(int(s) for s in first.data_shape)
    si = first.sampleinfo
    for obj in objs[1:]:
        other = tuple(int(s) for s in obj.data_shape)
        same = len(other) == len(shape) and all(a == b for i, (a, b) in enumerate(zip(shape, other)) if i != axis)
        n, m = si[:, 1] - si[:, 0], obj.sampleinfo[:, 1] - obj.sampleinfo[:, 0]
        if not same or n.shape != m.shape or not np.array_equal(n, m):
            raise SPYValueError("objects with matching shapes", "spy objects",
                                f"{shape} with trials of {n.tolist()} samples and {other} with trials of {m.tolist()} samples")
    if len(objs) > MAX_OBJECTS:
        raise SPYValueError(f"at most {MAX_OBJECTS} objects", "spy objects", f"{len(objs)} objects")
    # ---- what the reference does not ask for
    if dimord.index("time") != 0 or len(dimord) > 4:
        raise SPYValueError("data with time as its first dimension", varname="data", actual=f"dimord {dimord}")
    dtype = np.dtype(first.data_dtype)
    for i, obj in enumerate(objs):
        if np.dtype(obj.data_dtype) not in DTYPES:
            raise SPYTypeError(obj.data_dtype, varname=f"spy_obj{i + 1}", expected="float32, float64, complex64 or complex128 data")
        if np.dtype(obj.data_dtype) != dtype:
            raise SPYValueError("objects of one dtype (the operators can cast: `obj * 1.0`, `obj + 0j`)", "spy objects",
                                f"{dtype} and {np.dtype(obj.data_dtype)}")
    for i, obj in enumerate(objs):
        if obj.selection is not None:
            raise SPYValueError("objects without an in-place selection: make the selection a new object with "
                                "`spy.selectdata` first", varname=f"spy_obj{i + 1}", actual="active in-place selection")
    rows = []                                                    # per object the [start, stop) rows of its trials
    for obj in objs:
        info = obj.sampleinfo
        if np.any(info[:, 0] < 0) or np.any(info[:, 1] > obj.data_shape[0]) or np.any(info[:, 1] < info[:, 0]):
            raise SPYValueError("trials inside the data", varname="trialdefinition", actual=f"rows {info.tolist()}")
        rows.append([(int(a), int(b)) for a, b in info])
    n = (si[:, 1] - si[:, 0]).astype(np.int64)
    starts = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    trl = np.array(first.trialdefinition, dtype=float)
    trl[:, 0], trl[:, 1] = starts[:-1], starts[1:]
    nchan = [int(obj.data_shape[axis]) for obj in objs]
    labels = [getattr(obj, "channel", None) for obj in objs]
    joined = None
    if all(lab is not None and len(lab) == c for lab, c in zip(labels, nchan)):
        joined = np.concatenate([np.array(lab) for lab in labels])
        if len(set(str(c) for c in joined)) != joined.size:
            joined = None
    if joined is None:
        joined = _default_labels(first.__class__, sum(nchan))
    behind = int(np.prod(shape[axis + 1:], dtype=np.int64))
    log = {"dim": dim, "objects": len(objs), "channels": nchan}
    return types.SimpleNamespace(objs=list(objs), base=first, dtype=dtype, axis=axis, rows=rows, n=n, starts=starts[:-1],
                                 nrows=int(starts[-1]), pre=int(np.prod(shape[1:axis], dtype=np.int64)),
                                 run=[c * behind for c in nchan], inner=shape[1:axis] + (sum(nchan),) + shape[axis + 1:],
                                 full=[tuple(int(s) for s in obj.data_shape[1:]) for obj in objs],
                                 trialdefinition=trl, channel=joined, log=log)


def _new_object(plan):
    """the result object without its data: the first object's class, dimord, samplerate and labels, the joined channels"""
    base = plan.base
    out = base.__class__(None, samplerate=base.samplerate, dimord=base.dimord)
    out.trialdefinition = plan.trialdefinition
    for prop in ("freq", "taper"):
        if getattr(base, prop, None) is not None:
            setattr(out, prop, np.array(getattr(base, prop)))
    out.channel = plan.channel
    out.cfg = dict(base.cfg)
    out.cfg["concat"] = dict(plan.log)
    return out


def _chunks(plan, host, nbytes):
    """[k0, k1) trial ranges whose rows in the sources `host` (indices) take at most `nbytes` (at least one trial each);
    everything at once where no source needs an upload"""
    row_bytes = sum(int(np.prod(plan.full[s], dtype=np.int64)) for s in host) * plan.dtype.itemsize
    k0, acc = 0, 0
    for k, rows in enumerate(plan.n):
        if k > k0 and acc + int(rows) * row_bytes > nbytes:
            yield k0, k
            k0, acc = k, 0
        acc += int(rows) * row_bytes
    yield k0, len(plan.n)


# ---- the device part ------------------------------------------------------------------------------------------------------
def _run(plan, out):
    import torch
    from .arithmetic import _resident
    from .selectdata import _adopt
    from .. import backend
    backend.require_gpu()
    where = [_resident(obj) for obj in plan.objs]
    device = next((dev.device for dev, _ in where if dev is not None), None)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    where = [(dev, origin) if dev is not None and dev.device == device else (None, 0) for dev, origin in where]
    host = [s for s, (dev, _) in enumerate(where) if dev is None]
    tdtype = torch.from_numpy(np.empty(0, dtype=plan.dtype)).dtype
    res = torch.empty((plan.nrows,) + plan.inner, dtype=tdtype, device=device)
    for k0, k1 in _chunks(plan, host, CHUNK_BYTES):
        local = np.concatenate(([0], np.cumsum(plan.n[k0:k1]))).astype(np.int64)
        if local[-1] == 0:
            continue
        sources, first = [], []
        for s, (dev, origin) in enumerate(where):
            if dev is not None:                                   # read where it lies
                sources.append(dev)
                first.append(np.array([a - origin for a, _ in plan.rows[s][k0:k1]], dtype=np.int64))
                continue
            data = plan.objs[s].data                              # this chunk's trials, stacked
            stage = torch.empty((int(local[-1]),) + plan.full[s], dtype=tdtype, device=device)
            for k in range(k0, k1):
                a, b = plan.rows[s][k]
                if b > a:
                    stage[int(local[k - k0]):int(local[k - k0 + 1])].copy_(torch.from_numpy(np.ascontiguousarray(data[a:b])))
            sources.append(stage)
            first.append(local[:-1])
        backend.concat(sources, np.stack([plan.starts[k0:k1], plan.n[k0:k1]] + first, axis=1), res, plan.pre)
    _adopt(out, res, plan.dtype)


# ---- the front end ----------------------------------------------------------------------------------------------------------
def concat(spy_obj1, spy_obj2, *others, dim="channel"):
    """A new object of `spy_obj1`'s class whose trials hold the channels of `spy_obj1`, `spy_obj2` and up to six more
    objects side by side.  All objects need the same class, dimord, dtype, trial lengths and, away from the channel axis,
    shape.  Trial offsets, further columns of the trial definition, samplerate, `freq` and `taper` come from `spy_obj1`;
    the channel labels are joined where they are all distinct, else the class's default labels.  Only `dim="channel"`."""
    plan = _plan((spy_obj1, spy_obj2) + tuple(others), dim)
    out = _new_object(plan)
    _run(plan, out)
    return out
