"""Operator arithmetic on data objects: `data + 1`, `spec / baseline`, `a - b`, `2 / data`, `data ** 2`
(syncopy/datatype/methods/arithmetic.py: _parse_input :66-283, _perform_computation :305-413, arithmetic_cF), computed
on the device (csrc/arith.hip) over the selected trials, one launch per chunk of trials.

The arithmetic is NumPy's, `trial (op) operand` per selected trial; the result is a new object of the base's class whose
trials are stacked in selection order.  `_plan` is everything above the kernel (NumPy only: checks, result type, the
per-trial row table), `_run` the device part.  There is no CPU path.

Deviations from the reference, on purpose:
  * reflected operators keep their order: `2 - data` is 2 - x and `2 / data` is 2 / x (the reference computes data - 2
    and data / 2: base_data.py:1272-1285 passes no order); `0 / data` is allowed, only a zero divisor raises;
  * `**` with a complex base or a complex exponent raises NotImplementedError;
  * the data must be float32, float64, complex64 or complex128 (the reference lets NumPy promote integers);
  * an array operand that would enlarge a trial by broadcasting raises SPYValueError here, where the reference fails
    later, when it writes the larger trial into its dataset.
"""
import types

import numpy as np

from ..shared.errors import SPYTypeError, SPYValueError, SPYWarning

__all__ = []

# bytes of host trials that are on the device at once when the base (or the operand) has no device copy
CHUNK_BYTES = 512 << 20

DTYPES = tuple(np.dtype(t) for t in (np.float32, np.float64, np.complex64, np.complex128))
_REFLECTED = {"-": "rsub", "/": "rdiv"}
_DIRECT = {"+": "add", "-": "sub", "*": "mul", "/": "div", "**": "pow"}
# NumPy's fast paths of a scalar exponent (fast_scalar_power): x*x, a copy, ones, the square root, the reciprocal
_POWER_PATHS = {2.0: ("square", 0.0), 1.0: ("copy", 0.0), 0.0: ("ones", 0.0), 0.5: ("sqrt", 0.0), -1.0: ("rdiv", 1.0)}


# the operation and type codes of spyhip_arith (include/spyhip.h)
ARITH_OP = {"add": 0, "sub": 1, "mul": 2, "div": 3, "rsub": 4, "rdiv": 5, "pow": 6, "square": 7, "copy": 8, "ones": 9,
            "sqrt": 10}
ARITH_TYPE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.complex64): 2, np.dtype(np.complex128): 3}


def arith_view(array_shape, inner):
    """(extent, stride), four int64 each, of spyhip_arith's broadcast view: a contiguous array of `array_shape` seen as a
    trial (rows, *inner) with up to three inner axes; stride 0 where the array broadcasts"""
    shape = (1,) * (1 + len(inner) - len(array_shape)) + tuple(int(s) for s in array_shape)    # aligned with the trial
    shape = shape[:1] + (1,) * (3 - len(inner)) + shape[1:]
    inner = (1,) * (3 - len(inner)) + tuple(int(s) for s in inner)
    assert len(inner) == 3 and len(shape) == 4 and all(s in (1, e) for s, e in zip(shape[1:], inner))
    full = np.cumprod((shape[1:] + (1,))[::-1])[::-1]          # contiguous strides of the four axes
    stride = [int(full[i]) if shape[i] > 1 else 0 for i in range(4)]
    return np.array((shape[0],) + inner, dtype=np.int64), np.array(stride, dtype=np.int64)


def _process_operator(obj1, obj2, operator):
    """`obj1 (operator) obj2`, at least one of them a data object; operator: '+', '-', '*', '/' or '**'"""
    plan = _plan(obj1, obj2, operator)
    out = _new_object(plan)
    _run(plan, out)
    return out


# ---- checks and bookkeeping (NumPy only) -------------------------------------------------------------------------------
def _is_empty(obj):
    return (obj._data is None and obj._pending is None) or obj.trialdefinition is None


def _trial_layout(obj, varname):
    """(rows, chans, inner): the absolute [start, stop) rows of the selected trials, the selected channel indices (None:
    all of them) and the shape of one selected row"""
    from . import selected_channels, trial_rows
    if obj.dimord.index("time") != 0:
        raise SPYValueError("data with time as its first dimension", varname=varname, actual=f"dimord {obj.dimord}")
    inner = tuple(int(s) for s in obj.data_shape[1:])
    chans = selected_channels(obj) if "channel" in obj.dimord else None
    if chans is not None:
        if obj.dimord.index("channel") != len(obj.dimord) - 1:
            raise SPYValueError("data with channel as its last dimension", varname=varname, actual=f"dimord {obj.dimord}")
        chans = [int(c) for c in chans]
        if chans == list(range(inner[-1])):
            chans = None
        else:
            inner = inner[:-1] + (len(chans),)
    return trial_rows(obj), chans, inner


def _check_complex_operand(dtype, operand, kind, operator):
    if np.iscomplexobj(operand) != (dtype.kind == "c"):
        SPYWarning(f"Operand is {kind} of different mathematical type (real/complex)", caller=operator)


def _checked_dtype(dt, var, varname):
    if np.dtype(dt) not in DTYPES:
        raise SPYTypeError(var, varname=varname, expected="float32, float64, complex64 or complex128 data")
    return np.dtype(dt)


def _no_complex_power(operator, *dtypes):
    if operator == "**" and any(np.dtype(d).kind == "c" for d in dtypes):
        raise NotImplementedError("`**` with a complex base or a complex exponent is not implemented: "
                                  "powers take real data and a real exponent")


def _plan(obj1, obj2, operator):
    from . import _Base, SpikeData, selected_trialdefinition
    if operator not in _DIRECT:
        raise SPYValueError("supported arithmetic operator", actual=str(operator))
    reflected = not isinstance(obj1, _Base)
    base, operand = (obj2, obj1) if reflected else (obj1, obj2)
    if isinstance(base, SpikeData):
        raise SPYTypeError(base, varname="base", expected="`AnalogData`, `SpectralData` or `CrossSpectralData`")
    if _is_empty(base):
        raise SPYValueError("non-empty Syncopy data object", varname="base", actual="empty object")
    dtype = _checked_dtype(base.data_dtype, base.data_dtype, "base")
    rows, chans, inner = _trial_layout(base, "base")
    if len(rows) < 1:
        raise SPYValueError("at least 1 trial", varname="base", actual="got 0 trials")
    shapes = [(b - a,) + inner for a, b in rows]
    dtypes = [dtype] * len(rows)
    plan = types.SimpleNamespace(base=base, operand=operand, operator=operator, reflected=reflected, rows=rows, chans=chans,
                                 inner=inner, scalar=0.0, array=None, other=None, mode="scalar")
    op = _REFLECTED.get(operator, _DIRECT[operator]) if reflected else _DIRECT[operator]

    if isinstance(operand, _Base):
        opres = _plan_object(plan, dtype, shapes)
    elif np.issubdtype(type(operand), np.number):
        if np.isinf(operand):
            raise SPYValueError("finite scalar", varname="operand", actual=str(operand))
        if operator == "/" and not reflected and operand == 0:
            raise SPYValueError("non-zero scalar for division", varname="operand", actual=str(operand))
        _no_complex_power(operator, dtype, np.result_type(operand))
        _check_complex_operand(dtype, operand, "scalar", operator)
        opres = np.result_type(*dtypes, operand)
        plan.scalar = complex(operand) if np.iscomplexobj(operand) else float(operand)
        if op == "pow" and plan.scalar in _POWER_PATHS:
            op, plan.scalar = _POWER_PATHS[plan.scalar]
    elif isinstance(operand, (np.ndarray, list)):
        operand = np.array(operand)
        if operand.dtype.kind not in "iufc":
            raise SPYTypeError(operand, varname="operand", expected="array of numbers")
        _no_complex_power(operator, dtype, operand.dtype)
        _check_complex_operand(dtype, operand, "array", operator)
        opres = np.result_type(*dtypes, operand.dtype)
        for shape in shapes:
            try:
                ok = np.broadcast_shapes(shape, operand.shape) == shape
            except ValueError:
                ok = False
            if not ok:
                raise SPYValueError(f"array compatible to trial shape {shape}", varname="operand",
                                    actual=f"array with shape {operand.shape}")
        plan.mode = "array"
        plan.array = np.ascontiguousarray(operand.astype(_checked_dtype(opres, opres, "result")))
    else:
        raise SPYTypeError(operand, varname="operand", expected="Syncopy object, scalar or array-like")

    plan.op, plan.opres = op, _checked_dtype(opres, opres, "result")
    starts = np.concatenate(([0], np.cumsum([b - a for a, b in rows]))).astype(np.int64)
    plan.starts, plan.nrows = starts[:-1], int(starts[-1])
    trl = selected_trialdefinition(base)
    trl[:, 0], trl[:, 1] = starts[:-1], starts[1:]               # the result holds the stacked trials and nothing else
    plan.trialdefinition = trl
    opsel = operand.selection if isinstance(operand, _Base) else None
    plan.log = {"operator": operator, "base": base.__class__.__name__,
                "base selection": None if base.selection is None else dict(base.selection.select),
                "operand": operand.__class__.__name__,
                "operand selection": None if opsel is None else dict(opsel.select)}
    return plan


def _plan_object(plan, dtype, shapes):
    """the checks of a data-object operand (arithmetic.py:191-276); returns the result type"""
    base, operand, operator = plan.base, plan.operand, plan.operator
    if _is_empty(operand):
        raise SPYValueError("non-empty Syncopy data object", varname="operand", actual="empty object")
    if type(operand) is not type(base):
        raise SPYTypeError(operand, varname="operand", expected=f"Syncopy {base.__class__.__name__} object")
    if list(operand.dimord) != list(base.dimord):
        raise SPYValueError(f"dimord {base.dimord}", varname="operand", actual=f"dimord {operand.dimord}")
    if base.samplerate != operand.samplerate:
        raise SPYValueError("Syncopy objects with identical samplerate", varname="operand",
                            actual=f"Syncopy object with samplerates {base.samplerate} and {operand.samplerate}, "
                                   "respectively")
    if operand.selection is not None:
        SPYWarning("Found existing in-place selection in operand. "
                   "Shapes and trial counts of base and operand objects have to match up!", caller=operator)
    odtype = _checked_dtype(operand.data_dtype, operand.data_dtype, "operand")
    orows, ochans, oinner = _trial_layout(operand, "operand")
    if len(orows) != len(shapes):
        raise SPYValueError("Syncopy object with same number of trials (selected)", varname="operand",
                            actual=f"Syncopy object with {len(orows)} trials (selected)")
    if (dtype.kind == "c") != (odtype.kind == "c"):
        raise SPYTypeError(operand, varname="operand", expected="Syncopy data object of same numerical type (real/complex)")
    _no_complex_power(operator, dtype, odtype)
    opres = np.result_type(*([dtype] * len(shapes)), *([odtype] * len(orows)))
    oshapes = [(b - a,) + oinner for a, b in orows]
    if oshapes != shapes:
        raise SPYValueError(f"Syncopy object (selection) of compatible shapes {shapes}", varname="operand",
                            actual=f"Syncopy object (selection) with shapes {oshapes}")
    if operand.selection is not None:
        ids = list(operand.selection.trial_ids)
        picked = list(operand.selection.channel) if "channel" in operand.dimord else []
        if any(np.diff(sel).min() <= 0 for sel in (ids, picked) if len(sel) > 1):
            raise SPYValueError("Syncopy object with ordered unreverberated subset selection", varname="operand",
                                actual=f"Syncopy object with selection {operand.selection.select}")
    plan.mode = "object"
    plan.other = types.SimpleNamespace(base=operand, rows=orows, chans=ochans, inner=oinner)
    return opres


def _new_object(plan):
    """the result object without its data: class, dimord, trials and labels"""
    from . import selected_channel_labels
    base = plan.base
    out = base.__class__(None, samplerate=base.samplerate, dimord=base.dimord)
    out.trialdefinition = plan.trialdefinition
    for prop in ("freq", "taper", "channel_i", "channel_j"):
        if getattr(base, prop, None) is not None:
            setattr(out, prop, np.array(getattr(base, prop)))
    if getattr(base, "channel", None) is not None:
        out.channel = selected_channel_labels(base)
    out.cfg = dict(plan.log)
    return out


# ---- the device part ------------------------------------------------------------------------------------------------------
def _resident(obj):
    """(tensor, first host row it holds) of a device copy of obj.data that can be read now, or (None, 0)"""
    from . import AnalogData, CrossSpectralData
    from .. import backend, parallel
    if parallel.world()[1] > 1:
        return None, 0                     # under a process group every rank works from the host array
    want = np.dtype(obj.data_dtype)
    if isinstance(obj, AnalogData) and obj._device is not None and getattr(obj, "_upload", None) is None:
        if backend._NP_DTYPE.get(obj._device.dtype) == want:     # (a float64 recording is staged as float32: not that one)
            return obj._device, int(getattr(obj, "_row_origin", 0) or 0)
    dev = obj._dev if isinstance(obj, CrossSpectralData) else getattr(obj, "_resident", None)
    if dev is not None and tuple(dev.shape) == tuple(obj.data_shape) and backend._NP_DTYPE.get(dev.dtype) == want:
        return dev, 0
    return None, 0


def _host_chunks(src, nbytes):
    """[k0, k1) trial ranges of at most `nbytes` of the rows they upload (at least one trial each)"""
    row_bytes = int(np.prod(src.inner, dtype=np.int64)) * np.dtype(src.base.data_dtype).itemsize
    k0, acc = 0, 0
    for k, (a, b) in enumerate(src.rows):
        if k > k0 and acc + (b - a) * row_bytes > nbytes:
            yield k0, k
            k0, acc = k, 0
        acc += (b - a) * row_bytes
    yield k0, len(src.rows)


def _apply(op, src, starts, out, scalar=0.0, array=None, operand=None, operand_rows=None):
    """out[starts[k] ...] = trial k of `src` (op) operand, for all trials: in one launch from a device copy, else through
    uploads of CHUNK_BYTES"""
    import torch
    from .. import backend
    brow = starts if operand_rows is None else operand_rows
    n = np.array([b - a for a, b in src.rows], dtype=np.int64)
    dev, origin = _resident(src.base)
    if dev is not None:
        a0 = np.array([a - origin for a, _ in src.rows], dtype=np.int64)
        backend.arith(op, dev, np.stack([starts, a0, brow, n], axis=1), out, scalar, array, operand, chan=src.chans)
        return
    host = src.base.data
    for k0, k1 in _host_chunks(src, CHUNK_BYTES):
        local = np.concatenate(([0], np.cumsum(n[k0:k1])))
        stage = torch.empty((int(local[-1]),) + src.inner, dtype=torch.from_numpy(host[:0]).dtype, device=out.device)
        for k in range(k0, k1):
            a, b = src.rows[k]
            blk = host[a:b] if src.chans is None else np.take(host[a:b], src.chans, axis=-1)
            stage[int(local[k - k0]):int(local[k - k0 + 1])].copy_(torch.from_numpy(np.ascontiguousarray(blk)))
        backend.arith(op, stage, np.stack([starts[k0:k1], local[:-1], brow[k0:k1], n[k0:k1]], axis=1), out, scalar, array,
                      operand)


def _run(plan, out):
    import torch
    from . import AnalogData, CrossSpectralData
    from .. import backend
    backend.require_gpu()
    base = plan.base
    dev, _ = _resident(base)
    device = dev.device if dev is not None else torch.device("cuda", torch.cuda.current_device())
    tdtype = torch.from_numpy(np.empty(0, dtype=plan.opres)).dtype
    res = torch.empty((plan.nrows,) + plan.inner, dtype=tdtype, device=device)
    src = types.SimpleNamespace(base=base, rows=plan.rows, chans=plan.chans, inner=plan.inner)
    if plan.mode == "scalar":
        _apply(plan.op, src, plan.starts, res, scalar=plan.scalar)
    elif plan.mode == "array":
        _apply(plan.op, src, plan.starts, res, array=torch.from_numpy(plan.array).to(device))
    else:
        other = plan.other
        odev, origin = _resident(other.base)
        if odev is not None and odev.dtype == tdtype and other.chans is None and odev.device == device:
            orows = np.array([a - origin for a, _ in other.rows], dtype=np.int64)      # read where it lies
        else:                                                     # the operand's trials, stacked, in the result type
            odev, orows = torch.empty_like(res), plan.starts
            _apply("copy", other, plan.starts, odev)
        _apply(plan.op, src, plan.starts, res, operand=odev, operand_rows=orows)
    if isinstance(out, AnalogData) and plan.opres in (np.float32, np.complex64):
        out.adopt_device_result(res)
        return
    out.set_pending(lambda: backend.to_host(res), res.shape, plan.opres)
    if isinstance(out, CrossSpectralData):
        out._dev = res
    else:
        out._resident = res
