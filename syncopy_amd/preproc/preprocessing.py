"""`spy.preprocessing`: detrending, z-scoring, Butterworth and windowed-sinc filtering and rectification of AnalogData
along time (syncopy/preproc/preprocessing.py with preproc/compRoutines.py), on the device.

    spy.preprocessing(adata, freq=100)                                        # Butterworth low-pass, order 4, two-pass
    spy.preprocessing(adata, filter_class="firws", filter_type="bs", freq=[49, 51], order=2000)
    spy.preprocessing(adata, filter_class=None, polyremoval=1, zscore=True)

The front end validates, designs the filter on the host in float64 (design.py) and turns the request into the
reference's chain of steps: [detrend, z-score] if zscore, then [detrend, filter] (polyremoval is applied again by the
filter routine, as there), |.| fused into the last step.  All arithmetic on samples runs in csrc/preproc.hip; there is
no CPU path.  `compute_method="sequential"` with `routine_classes` swaps in a NumPy/SciPy model of the steps for the
tests.  Trials of equal length are filtered together, at most CHUNK_BYTES of input at a time; an input that already
lives on the device is not uploaded again, and the result stays on the device for a following spy.freqanalysis (the
host array is fetched when `.data` is first read).

Not implemented: `hilbert=<output>` (raises NotImplementedError after validation).  spy.resampledata lives in
resampledata.py.
"""
import numpy as np

from ..datatype import AnalogData, device_rows, selected_channels, selected_trialdefinition, trial_rows
from ..shared.errors import SPYInfo, SPYTypeError, SPYValueError, SPYWarning
from . import design

__all__ = ["preprocessing"]

availableFilters = ("but", "firws")
availableFilterTypes = design.FILTER_TYPES
availableDirections = ("twopass", "onepass", "onepass-minphase")
availableWindows = design.WINDOWS
hilbert_outputs = {"abs", "complex", "real", "imag", "absreal", "absimag", "angle"}

# bytes of input trials filtered at once (the work buffers on the device are a small multiple of this)
CHUNK_BYTES = 512 << 20


def _is_int_like(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and float(v) == int(v)


def _check_scalar(v, varname, lims, int_like=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise SPYTypeError(v, varname=varname, expected="scalar")
    if not np.isfinite(v) and not (np.isinf(v) and np.isinf(lims[1]) and v > 0 and not int_like):
        raise SPYValueError(f"value to be greater or equals {lims[0]} and less or equals {lims[1]}", varname=varname,
                            actual=str(v))
    if int_like and not _is_int_like(v):
        raise SPYValueError("integer-like value", varname=varname, actual=str(v))
    if v < lims[0] or v > lims[1]:
        raise SPYValueError(f"value to be greater or equals {lims[0]} and less or equals {lims[1]}", varname=varname,
                            actual=str(v))


def _check_freq(freq, filter_type, nyquist):
    if filter_type in ("lp", "hp"):
        _check_scalar(freq, "freq", [0, nyquist])
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
    hilbert      : validated, then refused with NotImplementedError (no inverse transform of arbitrary length yet)
    select       : in-place selection {"trials", "channel", "latency"}

    Returns float32 AnalogData with the input's dimord, channels and samplerate; `info["nan_trials"]` lists the trials
    whose input held a NaN when a filter or a detrending ran.  `chan_per_worker` / `parallel` are accepted and ignored."""
    if not isinstance(data, AnalogData):
        raise SPYTypeError(data, varname="data", expected="Syncopy AnalogData object")
    if (data._data is None and data._pending is None) or data.trialdefinition is None:
        raise SPYValueError("non-empty Syncopy data object", varname="data", actual="empty object")
    if data.dimord.index("time") != 0:
        raise SPYValueError("time x channel data", varname="data", actual=f"dimord {data.dimord}")
    defaults = dict(filter_class="but", filter_type="lp", freq=None, order=None, direction="twopass", window="hamming",
                    polyremoval=None, zscore=False, rectify=False, hilbert=False)
    given = dict(filter_class=filter_class, filter_type=filter_type, freq=freq, order=order, direction=direction,
                 window=window, polyremoval=polyremoval, zscore=zscore, rectify=rectify, hilbert=hilbert)
    unknown = set(kwargs) - {"chan_per_worker", "parallel"}
    if unknown:
        raise SPYValueError(f"one of {sorted(defaults)}", varname="kwargs", actual=str(sorted(unknown)))
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
            _check_scalar(order, "order", [0, np.inf], int_like=True)
            order = int(order)
    elif polyremoval is None and zscore is False:
        raise SPYValueError("a preprocessing method", varname="filter_class/polyremoval/zscore",
                            actual="neither filtering, detrending or zscore requested")
    if polyremoval is not None:
        _check_scalar(polyremoval, "polyremoval", [0, 1], int_like=True)
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

    had_selection = data.selection
    if select is not None:
        data.selectdata(select)
    try:
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
            raise NotImplementedError(f"hilbert='{hilbert}' is not implemented: it needs an inverse transform of "
                                      "arbitrary trial length on the device")

        if compute_method in (None, "hip"):
            out_data, nan_flags = _device_run(data, rows, pre, main or [], rectify)
        else:
            out_data, nan_flags = _model_run(data, rows, pre, main or [], rectify, routine_classes)

        out = AnalogData(None, samplerate=data.samplerate, dimord=data.dimord)
        out_data(out)
        out.trialdefinition = selected_trialdefinition(data)
        chans = selected_channels(data)
        out.channel = np.array(data.channel) if chans is None else np.array(data.channel)[chans]
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
    finally:
        data.selection = had_selection


def _host_trials(data, rows):
    chans = selected_channels(data)
    full = chans is None or list(chans) == list(range(data.data.shape[1]))
    return [data.data[a:b] if full else np.take(data.data[a:b], chans, axis=1) for a, b in rows]


def _model_run(data, rows, pre, main, rectify, ops):
    """The chain through a table of host functions (the tests' NumPy/SciPy model): ops[step name](trial, *args) ->
    trial, ops["has_nan"](trial) -> bool, ops["rectify"](trial) -> trial."""
    outs, flags = [], []
    for x in _host_trials(data, rows):
        x = np.array(x, dtype=np.float32)
        for step in pre:
            x = np.asarray(ops[step[0]](x, *step[1:]), dtype=np.float32)
        flags.append(bool(ops["has_nan"](x)) if main else False)
        for step in main:
            x = np.asarray(ops[step[0]](x, *step[1:]), dtype=np.float32)
        if rectify:
            x = np.asarray(ops["rectify"](x), dtype=np.float32)
        outs.append(x)
    arr = np.concatenate(outs, axis=0)

    def attach(out):
        out.data = arr
    return attach, flags


def _device_run(data, rows, pre, main, rectify):
    import torch
    from .. import backend
    backend.require_gpu()
    if data.data_dtype != np.float32:
        raise SPYTypeError(data.data_dtype, varname="data", expected="float32 data")
    steps = list(pre) + list(main)
    first_main = len(pre)
    chans = selected_channels(data)
    resident = data._device is not None and getattr(data, "_upload", None) is None
    src = data._device if resident else None
    src_rows = device_rows(data) if resident else rows
    nchan_in = int(data.data_shape[1])
    full = chans is None or list(chans) == list(range(nchan_in))
    nchan = nchan_in if full else len(chans)
    dev = src.device if resident else torch.device("cuda", torch.cuda.current_device())
    cidx = None if full else torch.as_tensor(list(chans), dtype=torch.int64, device=dev)
    lengths = [b - a for a, b in rows]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    res = torch.empty((int(starts[-1]), nchan), dtype=torch.float32, device=dev)
    flags = torch.zeros(len(rows), dtype=torch.int32, device=dev)
    taps_dev = {}
    groups = {}
    for k, n in enumerate(lengths):
        groups.setdefault(n, []).append(k)
    for n, members in groups.items():
        if n < 1:
            continue
        per = max(1, CHUNK_BYTES // (n * nchan * 4))
        for c0 in range(0, len(members), per):
            ks = members[c0:c0 + per]
            m = len(ks)
            # input: a view of the resident matrix when the chunk's trials follow each other there, else gathered
            if resident and full and all(src_rows[ks[i + 1]][0] == src_rows[ks[i]][1] for i in range(m - 1)):
                x = src[src_rows[ks[0]][0]:src_rows[ks[-1]][1]].view(m, n, nchan)
                owned = False
            elif resident:
                x = torch.stack([src[src_rows[k][0]:src_rows[k][1]] if full
                                 else src[src_rows[k][0]:src_rows[k][1]].index_select(1, cidx) for k in ks])
                owned = True
            else:
                host = data.data
                x = torch.empty((m, n, nchan), dtype=torch.float32, device=dev)
                for i, k in enumerate(ks):
                    a, b = rows[k]
                    blk = host[a:b] if full else np.take(host[a:b], chans, axis=1)
                    x[i].copy_(torch.from_numpy(np.ascontiguousarray(blk)))
                owned = True
            # output: straight into the result when the chunk's trials follow each other there
            direct = all(ks[i + 1] == ks[i] + 1 for i in range(m - 1))
            final = res[int(starts[ks[0]]):int(starts[ks[-1]] + n)].view(m, n, nchan) if direct else None
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
                else:
                    key = id(step[1])
                    if key not in taps_dev:
                        taps_dev[key] = torch.from_numpy(np.ascontiguousarray(step[1], dtype=np.float64)).to(dev)
                    backend.fir_same(cur, dst, taps_dev[key], nan, rect)
                if dst is not cur:
                    spare = cur if (cur is not x or owned) else None
                    cur = dst
            if final is None:
                for i, k in enumerate(ks):
                    res[int(starts[k]):int(starts[k] + n)].copy_(cur[i])
            flags[torch.as_tensor(ks, dtype=torch.int64, device=dev)] = nan_main
    flag_list = [bool(v) for v in flags.cpu().numpy()] if main else [False] * len(rows)
    shape = (int(starts[-1]), nchan)

    def attach(out):
        def fetch():
            arr = backend.to_host(res)
            out._device_key = (id(arr), arr.shape, tuple(out.dimord), str(dev), (0, arr.shape[0]))
            return arr
        out.set_pending(fetch, shape, np.float32)
        out._device = res                   # AnalogData.device_data() hands this out: no round trip before freqanalysis
        out._device_key = None
        out._row_origin = 0
        out.staged_rows = (0, shape[0])
    return attach, flag_list
