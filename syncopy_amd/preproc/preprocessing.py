"""`spy.preprocessing`: detrending, z-scoring, Butterworth and windowed-sinc filtering, rectification and the Hilbert
transform of AnalogData along time (syncopy/preproc/preprocessing.py with preproc/compRoutines.py), on the device.

    spy.preprocessing(adata, freq=100)                                        # Butterworth low-pass, order 4, two-pass
    spy.preprocessing(adata, filter_class="firws", filter_type="bs", freq=[49, 51], order=2000)
    spy.preprocessing(adata, filter_class=None, polyremoval=1, zscore=True)
    spy.preprocessing(adata, filter_type="bp", freq=[8, 12], hilbert="abs")   # band-pass, then the analytic amplitude

The front end validates, designs the filter on the host in float64 (design.py) and turns the request into the
reference's chain of steps: [detrend, z-score] if zscore, then [detrend, filter] (polyremoval is applied again by the
filter routine, as there), |.| fused into the last step, or the Hilbert transform as a last step of its own
(scipy.signal.hilbert over the trial length and the output conversion in one kernel, csrc/hilbert.hip).  All arithmetic
on samples runs in csrc/preproc.hip and csrc/hilbert.hip; there is no CPU path.  `compute_method="sequential"` with
`routine_classes` swaps in a NumPy/SciPy model of the steps for the tests.  Trials of equal length are filtered
together, at most CHUNK_BYTES of input at a time, and reach the device by the routes of shared/trial_chunks.py; the
result stays on the device for a following spy.freqanalysis (AnalogData.adopt_device_result).

spy.resampledata lives in resampledata.py.
"""
import numpy as np

from ..datatype import AnalogData, selected_channel_labels, selected_trialdefinition, trial_rows
from ..shared.errors import SPYInfo, SPYTypeError, SPYValueError, SPYWarning
from ..shared.trial_chunks import (ResultRows, TrialSource, applied_selection, check_analog_input, check_scalar,
                                   equal_length_chunks, reject_unknown_kwargs)
from . import design

__all__ = ["preprocessing"]

availableFilters = ("but", "firws")
availableFilterTypes = design.FILTER_TYPES
availableDirections = ("twopass", "onepass", "onepass-minphase")
availableWindows = design.WINDOWS
hilbert_outputs = {"abs", "complex", "real", "imag", "absreal", "absimag", "angle"}

# second-order sections the cascade kernels are compiled for (MAX_SECTIONS of csrc/preproc_kernel.h)
MAX_SECTIONS = 12

# longest trial the Hilbert kernels take (HILBERT_MAX_N of csrc/hilbert_route.h)
MAX_HILBERT_SAMPLES = 1 << 20

# bytes of input trials filtered at once (the work buffers on the device are a small multiple of this)
CHUNK_BYTES = 512 << 20


def _check_freq(freq, filter_type, nyquist):
    if filter_type in ("lp", "hp"):
        check_scalar(freq, "freq", [0, nyquist])
        return float(freq)
    try:
        arr = np.array(freq, dtype=float)
    except (TypeError, ValueError):
        raise SPYTypeError(freq, varname="freq", expected="array_like of two frequencies")
    if arr.shape != (2,):
        raise SPYValueError("array of shape (2,)", varname="freq", actual=f"shape = {arr.shape}")
    if not np.all(np.isfinite(arr)):
        raise SPYValueError("finite frequencies", varname="freq", actual=str(freq))
    if arr.min() < 0 or arr.max() > nyquist:
        raise SPYValueError(f"all array elements to be bounded by [0, {nyquist}]", varname="freq", actual=str(freq))
    if arr[0] == arr[1]:
        raise SPYValueError("two different frequencies", varname="freq", actual=freq)
    return np.sort(arr)


def preprocessing(data, filter_class="but", filter_type="lp", freq=None, order=None, direction="twopass",
                  window="hamming", polyremoval=None, zscore=False, rectify=False, hilbert=False, select=None,
                  compute_method=None, routine_classes=None, **kwargs):
    """Preprocessing of AnalogData with IIR and FIR filters.

    filter_class : "but" (Butterworth), "firws" (windowed sinc) or None (no filter)
    filter_type  : "lp", "hp", "bp" or "bs"
    freq         : cut-off frequency, or two of them for "bp" / "bs"
    order        : filter order; default 4 for "but", min(shortest trial, 1000) for "firws" (odd orders are raised by one)
    direction    : "twopass" (zero phase, forward and backward), "onepass", or "onepass-minphase" (firws only)
    window       : "hamming", "hann" or "blackman" (firws only)
    polyremoval  : 0 removes the mean, 1 the least-squares line, ahead of any filter
    zscore       : True standardizes every channel of every trial ahead of the filter
    rectify      : True returns |.| of the result
    hilbert      : "abs", "complex", "real", "imag", "absreal", "absimag" or "angle": that conversion of the analytic
                   signal (scipy.signal.hilbert along time, circular over each trial) of the result; not with `rectify`;
                   trials of at most 2^20 samples; a channel with a non-finite sample comes out all-NaN for that trial
    select       : in-place selection {"trials", "channel", "latency"}

    Returns float32 AnalogData (complex64 for hilbert="complex") with the input's dimord, channels and samplerate;
    `info["nan_trials"]` lists the trials whose input held a NaN when a filter, a detrending or the Hilbert step ran.
    `chan_per_worker` / `parallel` are accepted and ignored."""
    check_analog_input(data)
    defaults = dict(filter_class="but", filter_type="lp", freq=None, order=None, direction="twopass", window="hamming",
                    polyremoval=None, zscore=False, rectify=False, hilbert=False)
    given = dict(filter_class=filter_class, filter_type=filter_type, freq=freq, order=order, direction=direction,
                 window=window, polyremoval=polyremoval, zscore=zscore, rectify=rectify, hilbert=hilbert)
    reject_unknown_kwargs(kwargs, defaults)
    new_cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in given.items()}
    if select is not None:
        new_cfg["select"] = select

    if filter_class is not None:
        if filter_class not in availableFilters:
            raise SPYValueError("'but' or 'firws'", varname="filter_class", actual=filter_class)
        if not isinstance(filter_type, str) or filter_type not in availableFilterTypes:
            raise SPYValueError(f"one of {availableFilterTypes}", varname="filter_type", actual=filter_type)
        freq = _check_freq(freq, filter_type, data.samplerate / 2)
        if order is not None:
            check_scalar(order, "order", [0, np.inf], int_like=True)
            order = int(order)
    elif polyremoval is None and zscore is False:
        raise SPYValueError("a preprocessing method", varname="filter_class/polyremoval/zscore",
                            actual="neither filtering, detrending or zscore requested")
    if polyremoval is not None:
        check_scalar(polyremoval, "polyremoval", [0, 1], int_like=True)
        polyremoval = int(polyremoval)
    if not isinstance(zscore, bool):
        raise SPYValueError("either `True` or `False`", varname="zscore", actual=zscore)
    if not isinstance(rectify, bool):
        raise SPYValueError("either `True` or `False`", varname="rectify", actual=rectify)
    if rectify and hilbert:
        raise SPYValueError("either rectification or Hilbert transform", varname="rectify/hilbert",
                            actual=(rectify, hilbert))
    if hilbert and hilbert not in hilbert_outputs:
        raise SPYValueError(f"one of {hilbert_outputs}", varname="hilbert", actual=hilbert)

    with applied_selection(data, select):
        rows = trial_rows(data)
        if len(rows) < 1:
            raise SPYValueError("at least 1 trial", varname="data", actual="got 0 trials")
        lengths = np.array([b - a for a, b in rows])
        detrend = [("detrend", polyremoval)] if polyremoval is not None else []
        pre = detrend + [("standardize",)] if zscore else []
        main = None

        if filter_class == "but":
            if window != defaults["window"] and window is not None:
                raise SPYValueError("no `window` setting for IIR filtering", varname="window", actual=window)
            if direction is None:
                direction = "twopass"
                SPYInfo(f"Setting default direction for IIR filter to '{direction}'")
            elif not isinstance(direction, str) or direction not in ("onepass", "twopass"):
                raise SPYValueError("'onepass' or 'twopass'", varname="direction", actual=direction)
            if order is None:
                order = 4
            if order < 1:
                raise SPYValueError("order of at least 1", varname="order", actual=str(order))
            sos, zi, edge = design.butterworth(order, freq, filter_type, data.samplerate)
            if sos.shape[0] > MAX_SECTIONS:          # refused here, ahead of any upload: the launchers would refuse too
                raise SPYValueError(f"a filter of at most {MAX_SECTIONS} second-order sections (order {2 * MAX_SECTIONS} "
                                    f"for 'lp' / 'hp', {MAX_SECTIONS} for 'bp' / 'bs')", varname="order", actual=str(order))
            if direction == "twopass":
                if lengths.min() <= edge:
                    raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
                main = detrend + [("sosfiltfilt", sos, zi, edge)]
            else:
                main = detrend + [("sosfilt", sos)]
        elif filter_class == "firws":
            if window not in availableWindows:
                raise SPYValueError("'hamming' or 'hann' or 'blackman'", varname="window", actual=window)
            if direction is None:
                direction = "onepass"
                SPYInfo(f"Setting default direction for FIR filter to '{direction}'")
            elif not isinstance(direction, str) or direction not in availableDirections:
                raise SPYValueError("'twopass' or 'onepass' or 'onepass-minphase'", varname="direction",
                                    actual=direction)
            if order is None:
                order = int(lengths.min()) if lengths.min() < 1000 else 1000
                SPYInfo(f"Setting order for FIR filter to {order}")
            taps = design.windowed_sinc(window, order, freq / data.samplerate, filter_type)
            if direction == "onepass-minphase":
                taps = design.minimum_phase(taps)
            main = detrend + [("fir", taps)] * (2 if direction == "twopass" else 1)
        elif polyremoval is not None and zscore is False:
            main = list(detrend)
        if hilbert:
            if lengths.max() > MAX_HILBERT_SAMPLES:     # refused here, ahead of any upload: the plan would refuse too
                raise SPYValueError(f"trials of at most {MAX_HILBERT_SAMPLES} (2^20) samples for the Hilbert transform",
                                    varname="data", actual=f"a trial of {int(lengths.max())} samples")
            if compute_method not in (None, "hip") and "hilbert" not in (routine_classes or {}):
                raise NotImplementedError(f"hilbert='{hilbert}': the routine table has no 'hilbert' entry")
            main = (main or []) + [("hilbert", hilbert)]

        out = AnalogData(None, samplerate=data.samplerate, dimord=data.dimord)
        if compute_method in (None, "hip"):
            res, nan_flags = _device_run(data, rows, pre, main or [], rectify)
            out.adopt_device_result(res)            # stays on the device: no round trip before a spy.freqanalysis
        else:
            out.data, nan_flags = _model_run(data, rows, pre, main or [], rectify, routine_classes)
        out.trialdefinition = selected_trialdefinition(data)
        out.channel = selected_channel_labels(data)
        if main is not None:
            nan_trials = [int(k) for k, f in enumerate(nan_flags) if f]
            if nan_trials:
                msg = "Data contains NaNs! See `.info['nan_trials']` for the offending trials"
                if filter_class == "but":
                    msg += "\n\t\t try using a 'onepass' FIR filter of low order.."
                SPYWarning(msg)
            out.info["nan_trials"] = nan_trials
        out.cfg = dict(getattr(data, "cfg", {}) or {})
        out.cfg["preprocessing"] = new_cfg
        return out


def _model_run(data, rows, pre, main, rectify, ops):
    """The chain through a table of host functions (the tests' NumPy/SciPy model): ops[step name](trial, *args) ->
    trial, ops["has_nan"](trial) -> bool, ops["rectify"](trial) -> trial."""
    outs, flags = [], []
    for x in TrialSource(data, rows).host_trials():
        x = np.array(x, dtype=np.float32)
        for step in pre:
            x = np.asarray(ops[step[0]](x, *step[1:]), dtype=np.float32)
        flags.append(bool(ops["has_nan"](x)) if main else False)
        for step in main:
            x = np.asarray(ops[step[0]](x, *step[1:]))
            if not (step[0] == "hilbert" and np.iscomplexobj(x)):        # hilbert="complex" stays complex64
                x = x.astype(np.float32, copy=False)
        if rectify:
            x = np.asarray(ops["rectify"](x), dtype=np.float32)
        outs.append(x)
    return np.concatenate(outs, axis=0), flags


def _device_run(data, rows, pre, main, rectify):
    import torch
    from .. import backend
    backend.require_gpu()
    if data.data_dtype != np.float32:
        raise SPYTypeError(data.data_dtype, varname="data", expected="float32 data")
    steps = list(pre) + list(main)
    first_main = len(pre)
    source = TrialSource(data, rows)
    nchan, dev = source.nchan, source.dev
    lengths = [b - a for a, b in rows]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    hilbert = steps[-1][1] if steps and steps[-1][0] == "hilbert" else None
    res = torch.empty((int(starts[-1]), nchan), dtype=torch.complex64 if hilbert == "complex" else torch.float32,
                      device=dev)
    result = ResultRows(starts, res)
    flags = torch.zeros(len(rows), dtype=torch.int32, device=dev)
    taps_dev = {}
    for n, ks in equal_length_chunks(lengths, nchan, CHUNK_BYTES):
        m = len(ks)
        x, owned = source.gather(ks, n)             # not owned: a view of the resident input, never written into
        final = result.view(ks, n)                  # the last step writes straight into the result where it can
        spare = None
        nan_pre = torch.zeros(m, dtype=torch.int32, device=dev)
        nan_main = torch.zeros(m, dtype=torch.int32, device=dev)
        cur = x
        for j, step in enumerate(steps):
            last = j == len(steps) - 1
            nan = nan_main if j >= first_main else nan_pre
            in_place_ok = step[0] in ("detrend", "sosfilt", "sosfiltfilt") and (owned or cur is not x)
            if last and final is not None:
                dst = final
            elif last and hilbert == "complex":
                dst = torch.empty((m, n, nchan), dtype=torch.complex64, device=dev)
            elif in_place_ok:
                dst = cur
            else:
                if spare is None or spare is cur:
                    spare = torch.empty((m, n, nchan), dtype=torch.float32, device=dev)
                dst = spare
            rect = rectify and last
            if step[0] == "detrend":
                backend.detrend(cur, dst, step[1], nan, rect)
            elif step[0] == "standardize":
                backend.standardize(cur, dst, nan, rect)
            elif step[0] == "sosfilt":
                backend.sosfilt(cur, dst, step[1], nan, rect)
            elif step[0] == "sosfiltfilt":
                backend.sosfiltfilt(cur, dst, step[1], step[2], step[3], nan, rect)
            elif step[0] == "hilbert":
                backend.hilbert(cur, dst, step[1], nan)
            else:
                key = id(step[1])
                if key not in taps_dev:
                    taps_dev[key] = torch.as_tensor(np.ascontiguousarray(step[1], dtype=np.float64), device=dev)
                backend.fir_same(cur, dst, taps_dev[key], nan, rect)
            if dst is not cur:
                spare = cur if (cur is not x or owned) else None
                cur = dst
        if final is None:
            result.scatter(ks, n, cur)
        flags[torch.as_tensor(ks, dtype=torch.int64, device=dev)] = nan_main
    flag_list = [bool(v) for v in flags.cpu().numpy()] if main else [False] * len(rows)
    return res, flag_list
