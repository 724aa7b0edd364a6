"""`spy.mean`, `spy.var`, `spy.std`, `spy.median` and `spy.itc`: summary statistics along a dimension of a data object
or over its trials (syncopy/statistics/summary_stats.py:24-205, 321-486 and statistics/compRoutines.py:22-143), on the
device.

    spy.mean(data, dim="trials")                  # one trial: the sequential sum over the trials in the data's own
                                                  # dtype, then ONE division (summary_stats.py:321-400, :408-428)
    spy.mean(data, dim="time" | "freq" | "channel" | ..., keeptrials=True)
                                                  # np.nanmean(trial, axis, keepdims=True) per trial
                                                  # (compRoutines.py:22-57), then the usual trial average
                                                  # (computational_routine.py:1022-1032) if keeptrials=False

Both run as kernels of libspyhip (`spyhip_trial_mean_f32`: one thread per element walks the trials in order - the
reference's rounding sequence, bit for bit; `spyhip_axis_nanmean`: NumPy's summation order along the axis); there is no
CPU path.  `compute_method="sequential"` with `routine_classes` swaps in the oracle's NumPy functions for the tests.

var / std / median follow the same rules with np.nanvar / np.nanstd / np.nanmedian per trial (csrc/stats.hip); over the
trials, var and std are the reference's sequential two-pass variance in the data's dtype and the median is not supported
(summary_stats.py:382).  `spy.itc` is the inter-trial coherence of complex spectra: |mean over trials and tapers of
z / |z||.  The trial passes stream the trials to the device in chunks of at most CHUNK_BYTES and carry their
accumulators across chunks, so device memory does not grow with the trial count.
"""
import numpy as np

from ..datatype import AnalogData, CrossSpectralData, SpectralData
from ..shared.errors import SPYTypeError, SPYValueError

__all__ = ["mean", "var", "std", "median", "itc"]

_DIMPROPS = ("channel", "freq", "taper", "channel_i", "channel_j")

# bytes of trials held on the device at once by the trial passes of var / std / itc
CHUNK_BYTES = 512 << 20


def _selected_trials(data):
    """[(trial array, absolute trial id)] honouring an in-place selection (trials in the given order, channels of
    AnalogData / SpectralData along their channel axis, latency windows along time)."""
    sel = data.selection
    trials = data.trials
    ids = list(range(len(trials))) if sel is None else list(sel.trial_ids)
    out = []
    for t in ids:
        x = trials[t]
        if sel is not None:
            a, b = sel.time[t]
            tax = data.dimord.index("time")
            if (a, b) != (0, x.shape[tax]):
                idx = [slice(None)] * x.ndim
                idx[tax] = slice(a, b)
                x = x[tuple(idx)]
            if "channel" in data.dimord and list(sel.channel) != list(range(x.shape[data.dimord.index("channel")])):
                x = np.take(x, sel.channel, axis=data.dimord.index("channel"))
        out.append((x, t))
    return out


def _new_like(data, arr, trialdefinition, dim=None, trials_sel=None, op="mean", skip=()):
    cls = data.__class__
    if cls is AnalogData:
        out = AnalogData(arr, samplerate=data.samplerate, trialdefinition=trialdefinition, dimord=data.dimord)
    else:
        out = cls(arr, samplerate=data.samplerate, trialdefinition=trialdefinition, dimord=data.dimord)
    for prop in _DIMPROPS:
        if prop in skip or not hasattr(data, prop) or getattr(data, prop) is None:
            continue
        val = np.asarray(getattr(data, prop))
        if prop == "channel" and data.selection is not None:
            val = val[list(data.selection.channel)]
        if dim is not None and dim in prop:
            # the averaged dimension: one entry labelled with the operation; a numerical freq axis is gone
            # (compRoutines.py:131-141 - `dim in prop`, so dim="channel" also relabels channel_i / channel_j)
            setattr(out, prop, None if dim == "freq" else np.array([op]))
            continue
        setattr(out, prop, val)
    out.cfg = dict(getattr(data, "cfg", {}) or {})
    return out


def mean(spy_data, dim, keeptrials=True, select=None, compute_method=None, routine_classes=None, **kwargs):
    """Average of `spy_data` along the dimension `dim` (a label of its dimord) or over its trials (dim="trials").

    spy_data   : AnalogData, SpectralData or CrossSpectralData
    dim        : "trials" or one of spy_data.dimord
    keeptrials : False additionally averages the per-trial results over the trials (no effect for dim="trials")
    select     : in-place selection {"trials", "channel", "latency"}

    Returns a new object of the same class.  Trial averages need trials of identical shape
    (summary_stats.py:259-266)."""
    return _statistic(spy_data, dim, "mean", keeptrials, select, compute_method, routine_classes)


def var(spy_data, dim, keeptrials=True, select=None, compute_method=None, routine_classes=None, **kwargs):
    """Variance (ddof 0) of `spy_data` along the dimension `dim` or over its trials (dim="trials"); arguments as for
    `mean`.  Along a dimension NaNs are skipped (np.nanvar); over the trials they are not (summary_stats.py:431-456).
    The result has the data's dtype (complex data: the imaginary part is 0)."""
    _check_device_dtype(spy_data, compute_method)
    return _statistic(spy_data, dim, "var", keeptrials, select, compute_method, routine_classes)


def std(spy_data, dim, keeptrials=True, select=None, compute_method=None, routine_classes=None, **kwargs):
    """Standard deviation (ddof 0): the square root of `var`; arguments as for `mean`."""
    _check_device_dtype(spy_data, compute_method)
    return _statistic(spy_data, dim, "std", keeptrials, select, compute_method, routine_classes)


def median(spy_data, dim, keeptrials=True, select=None, compute_method=None, routine_classes=None, **kwargs):
    """Median of `spy_data` along the dimension `dim` (np.nanmedian; complex values ordered by real, then imaginary
    part); arguments as for `mean`.  The median over trials raises NotImplementedError, as in the reference
    (summary_stats.py:380-382)."""
    _check_device_dtype(spy_data, compute_method)
    return _statistic(spy_data, dim, "median", keeptrials, select, compute_method, routine_classes)


def itc(spec_data, select=None, compute_method=None, routine_classes=None, **kwargs):
    """Inter-trial coherence of complex SpectralData (spy.freqanalysis(..., output="fourier")): the length of the mean
    unit vector z / |z| over the trials and then the tapers (summary_stats.py:156-205, 364-377, 459-486).

    Returns float32 SpectralData with one trial and a taper axis of length 1; a time-frequency spectrum keeps its time
    axis.  All selected trials need the same shape; a zero bin gives NaN."""
    if not isinstance(spec_data, SpectralData):
        raise SPYTypeError(spec_data, varname="spec_data", expected="SpectralData")
    if spec_data.data is None or spec_data.trialdefinition is None:
        raise SPYValueError("non-empty Syncopy data object", varname="spec_data", actual="empty object")
    if not np.iscomplexobj(spec_data.data):
        raise SPYValueError("complex valued spectra, set `output='fourier` in spy.freqanalysis!", varname="spec_data",
                            actual="real valued spectral data")
    _check_device_dtype(spec_data, compute_method)
    had_selection = spec_data.selection
    if select is not None:
        spec_data.selectdata(select)
    try:
        trials = _selected_trials(spec_data)
        _check_equal_trials(trials)
        seldef = (spec_data.trialdefinition if spec_data.selection is None else spec_data.selection.trialdefinition)
        ops = _device_ops() if compute_method in (None, "hip") else routine_classes
        res = ops["itc"]([x for x, _ in trials], spec_data.dimord.index("taper"))
        trldef = np.array(seldef[0, :], dtype=float)[None, :]
        trldef[0, :2] = [0, res.shape[spec_data.dimord.index("time")]]
        return _new_like(spec_data, res, trldef, dim=None, skip=("taper",))      # taper labels not carried (:377)
    finally:
        spec_data.selection = had_selection


def _check_device_dtype(data, compute_method):
    """The device kernels take float32 / complex64 only: other dtypes fail before any device work."""
    dt = getattr(getattr(data, "data", None), "dtype", None)
    if compute_method in (None, "hip") and dt is not None and dt not in (np.float32, np.complex64):
        raise SPYTypeError(dt, varname="data", expected="float32 or complex64 data")


def _check_equal_trials(trials):
    if len(trials) < 1:
        raise SPYValueError("at least 1 trial", varname="in_data", actual=f"got {len(trials)} trials")
    shape0 = trials[0][0].shape
    for x, _ in trials:
        if x.shape != shape0:
            raise SPYValueError("all trials to have the same shape", varname="in_data",
                                actual=f"found trials of different shape: {shape0} and {x.shape}")


def _statistic(spy_data, dim, op, keeptrials, select, compute_method, routine_classes):
    if not isinstance(spy_data, (AnalogData, SpectralData, CrossSpectralData)):
        raise SPYTypeError(spy_data, varname="spy_data", expected="Syncopy data object")
    if spy_data.data is None or spy_data.trialdefinition is None:
        raise SPYValueError("non-empty Syncopy data object", varname="spy_data", actual="empty object")
    if dim != "trials" and dim not in spy_data.dimord:
        raise SPYValueError(f"one of {spy_data.dimord} or 'trials'", varname="dim", actual=str(dim))
    had_selection = spy_data.selection
    if select is not None:
        spy_data.selectdata(select)
    try:
        trials = _selected_trials(spy_data)
        if len(trials) < 1:
            raise SPYValueError("at least 1 trial", varname="in_data", actual=f"got {len(trials)} trials")
        seldef = (spy_data.trialdefinition if spy_data.selection is None else spy_data.selection.trialdefinition)
        ops = _device_ops() if compute_method in (None, "hip") else routine_classes
        if dim == "trials":
            _check_equal_trials(trials)
            if op == "median":
                raise NotImplementedError("Trial median not supported at the moment")     # summary_stats.py:380-382
            res = ops["trial_" + op]([x for x, _ in trials])
            trldef = np.array(seldef[0, :], dtype=float)[None, :]
            trldef[0, :2] = [0, res.shape[spy_data.dimord.index("time")]]
            return _new_like(spy_data, res, trldef, dim=None)
        axis = spy_data.dimord.index(dim)
        per_trial = [ops["axis_" + op](x, axis) for x, _ in trials]
        tax = spy_data.dimord.index("time")
        if not keeptrials:
            shape0 = per_trial[0].shape
            if any(r.shape != shape0 for r in per_trial):
                raise NotImplementedError("trial averaging needs trials of equal length")      # computational_routine.py:319-321
            res = ops["trial_mean"](per_trial)
            n = res.shape[tax]
            trldef = np.array([[0, 1, 0]], dtype=float) if dim == "time" else np.array([[0, n, seldef[0, 2]]], dtype=float)
            return _new_like(spy_data, res, trldef, dim=dim, op=op)
        res = np.concatenate(per_trial, axis=tax)
        if dim == "time":
            k = np.arange(len(per_trial), dtype=float)[:, None]
            trldef = np.hstack((k, k + 1, np.zeros((len(per_trial), 1))))
        else:
            trldef = np.array(seldef, dtype=float)
        return _new_like(spy_data, res, trldef, dim=dim, op=op)
    finally:
        spy_data.selection = had_selection


def _device_ops():
    import torch
    from .. import backend
    backend.require_gpu()

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def checked(x):
        d = to_dev(x)
        if d.dtype not in (torch.float32, torch.complex64):
            raise SPYTypeError(d.dtype, varname="data", expected="float32 or complex64 data")
        return d

    def trial_mean(trials):
        return backend.to_host(backend.trial_mean(torch.stack([checked(x) for x in trials]).contiguous()))

    def axis_mean(x, axis):
        return backend.to_host(backend.axis_nanmean(checked(x), axis))

    def upload(trials):
        first = checked(trials[0])
        out = torch.empty((len(trials),) + tuple(first.shape), dtype=first.dtype, device=first.device)
        out[0].copy_(first)
        for j in range(1, len(trials)):
            out[j].copy_(torch.from_numpy(np.ascontiguousarray(trials[j])))
        return out

    def chunks(trials):
        """the trials on the device, CHUNK_BYTES at a time (at least one trial per chunk)"""
        per = max(1, CHUNK_BYTES // max(1, trials[0].nbytes))
        for a in range(0, len(trials), per):
            yield upload(trials[a:a + per])

    def trial_moment(trials, take_sqrt):
        T = len(trials)
        one = CHUNK_BYTES // max(1, trials[0].nbytes) >= T
        x = upload(trials) if one else None
        dtype = checked(trials[0][:0]).dtype
        acc = torch.zeros(trials[0].shape, dtype=dtype, device="cuda")
        for c in ([x] if one else chunks(trials)):
            backend.trial_sum(c, acc)
        mean = backend.trial_sum_finalize(acc, T)
        sq = torch.zeros(trials[0].shape, dtype=torch.float32, device="cuda")
        for c in ([x] if one else chunks(trials)):                 # one upload when the selection fits one chunk
            backend.trial_sqdev(c, mean, sq)
        return backend.to_host(backend.trial_var_finalize(sq, T, dtype, take_sqrt))

    def itc(trials, taper_axis):
        acc = torch.zeros(trials[0].shape, dtype=torch.complex64, device="cuda")
        for c in chunks(trials):
            backend.itc_accumulate(c, acc)
        return backend.to_host(backend.itc_finalize(acc, len(trials), taper_axis))

    return {"trial_mean": trial_mean, "axis_mean": axis_mean,
            "trial_var": lambda trials: trial_moment(trials, False),
            "trial_std": lambda trials: trial_moment(trials, True),
            "axis_var": lambda x, axis: backend.to_host(backend.axis_nanvar(checked(x), axis)),
            "axis_std": lambda x, axis: backend.to_host(backend.axis_nanvar(checked(x), axis, take_sqrt=True)),
            "axis_median": lambda x, axis: backend.to_host(backend.axis_nanmedian(checked(x), axis)),
            "itc": itc}
