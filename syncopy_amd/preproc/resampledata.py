"""`spy.resampledata`: rational resampling and downsampling of AnalogData along time (syncopy/preproc/resampledata.py
with preproc/resampling.py and the Resample / Downsample routines of preproc/compRoutines.py), on the device.

    spy.resampledata(adata, resamplefs=600)                                       # 1 kHz -> 600 Hz, anti-alias included
    spy.resampledata(adata, resamplefs=250, method="downsample", lpfreq=125)      # low-pass, then every 4th sample

method="resample": (up, down) = Fraction(resamplefs / samplerate).limit_denominator(), the anti-alias filter is the
Hamming windowed sinc of design.py at `lpfreq` (default: the new Nyquist) divided by up, and every trial becomes
scipy.signal.resample_poly(trial, up, down, window=taps) - one pass of the up-FIR-down kernel (csrc/resample.hip).
method="downsample": trial[::samplerate // resamplefs], after the two-pass windowed-sinc low-pass of spy.preprocessing
when `lpfreq` is given; the second pass of that filter computes only the samples that are kept.  There is no CPU path;
`compute_method="sequential"` with `routine_classes` swaps in a NumPy/SciPy model of the steps for the tests.  Trials of
equal length go through the kernel together, at most CHUNK_BYTES of input at a time, and reach the device by the routes
of shared/trial_chunks.py; the result stays on the device for a following spy.freqanalysis.

Deviations from the reference, on purpose:
  * lpfreq=0 with method="resample" raises SPYValueError (there a zero cut-off silently falls through to SciPy's Kaiser
    design);
  * a trial of n samples gives ceil(n * up / down) samples, the length of resample_poly, also where the reference's float
    ceil(n * resamplefs / samplerate) differs from it (there the reference cannot store its own result);
  * the sample ranges of the output's trial definition are those of the stacked rows (cumulative lengths), the offsets
    ceil(offset * resamplefs / samplerate).  For trials that tile the data from row 0 that is the reference's
    _resampling_trl_definition wherever its own ranges tile the stacked rows; its ranges can overlap by one row for odd
    trial starts, which is not reproduced;
  * float32 input only, and time must be the first axis, as in spy.preprocessing.
"""
from fractions import Fraction

import numpy as np

from ..datatype import AnalogData, selected_channel_labels, selected_trialdefinition, trial_rows
from ..shared.errors import SPYTypeError, SPYValueError, SPYWarning
from ..shared.trial_chunks import (ResultRows, TrialSource, applied_selection, check_analog_input, check_scalar,
                                   equal_length_chunks, reject_unknown_kwargs)
from . import design

__all__ = ["resampledata"]

availableMethods = ("downsample", "resample")

# bytes of input trials resampled at once
CHUNK_BYTES = 512 << 20


def resampledata(data, resamplefs=1.0, method="resample", lpfreq=None, order=None, select=None, compute_method=None,
                 routine_classes=None, **kwargs):
    """Resampling or downsampling of AnalogData.

    resamplefs : the new sampling rate, in [1, data.samplerate]; an integer division of it for "downsample"
    method     : "resample" (any rational ratio, anti-alias filter included) or "downsample" (every n-th sample)
    lpfreq     : cut-off of the anti-alias low-pass in Hz, in [0, resamplefs / 2]; None is the new Nyquist for
                 "resample" and no filter at all for "downsample"
    order      : order of that filter; default min(shortest trial, 1000) (odd orders are raised by one)
    select     : in-place selection {"trials", "channel", "latency"}

    Returns float32 AnalogData with the input's dimord, the selected channels, samplerate = resamplefs and the trials
    stacked in order (the trial definition and the deviations from the reference: module docstring).
    `chan_per_worker` / `parallel` are accepted and ignored."""
    if method not in availableMethods:
        raise SPYValueError("'downsample' or 'resample'", varname="method", actual=method)
    check_analog_input(data)
    new_cfg = dict(resamplefs=resamplefs, method=method, lpfreq=lpfreq, order=order)
    reject_unknown_kwargs(kwargs, new_cfg)
    if select is not None:
        new_cfg["select"] = select
    samplerate = float(data.samplerate)
    check_scalar(resamplefs, "resamplefs", [1, samplerate])
    if order is not None:
        check_scalar(order, "order", [0, np.inf], int_like=True)
        order = int(order)
        if order < 100:
            SPYWarning(f"You have chosen an anti-alias filter of very low `order={order}`, expect a slow roll-off!")
    if lpfreq is not None:
        check_scalar(lpfreq, "lpfreq", [0, resamplefs / 2])
    if method == "downsample":
        if samplerate % resamplefs != 0:
            raise SPYValueError("integer division of the original sampling rate for `method='downsample'`",
                                varname="resamplefs", actual=resamplefs)
    else:
        if lpfreq is not None and lpfreq == 0:
            raise SPYValueError("a cut-off frequency above 0 for `method='resample'`", varname="lpfreq", actual=lpfreq)
        if samplerate % resamplefs == 0:
            SPYWarning("New sampling rate is integeger division of the original sampling rate, "
                       "consider using `method='downsample'`")

    with applied_selection(data, select):
        rows = trial_rows(data)
        if len(rows) < 1:
            raise SPYValueError("at least 1 trial", varname="data", actual="got 0 trials")
        lengths = np.array([b - a for a, b in rows], dtype=np.int64)
        if order is None:
            order = int(lengths.min()) if lengths.min() < 1000 else 1000

        if method == "resample":
            frac = Fraction.from_float(resamplefs / samplerate).limit_denominator()
            up, down = frac.numerator, frac.denominator
            f_c = 0.5 * resamplefs / samplerate if lpfreq is None else lpfreq / samplerate
            taps = design.windowed_sinc("hamming", order, f_c / up) * up
            steps = [("resample", taps, up, down)]
            out_lengths = (lengths * up + down - 1) // down
        else:
            skip = int(samplerate // resamplefs)
            steps = []
            if lpfreq is not None:
                taps = design.windowed_sinc("hamming", order, lpfreq / samplerate)
                steps = [("fir", taps), ("fir", taps)]
            steps.append(("downsample", skip))
            out_lengths = (lengths + skip - 1) // skip

        out = AnalogData(None, samplerate=float(resamplefs), dimord=data.dimord)
        if compute_method in (None, "hip"):
            # the result stays on the device: no round trip before a spy.freqanalysis
            out.adopt_device_result(_device_run(data, rows, steps, out_lengths))
        else:
            out.data = _model_run(data, rows, steps, out_lengths, routine_classes)
        edges = np.concatenate([[0], np.cumsum(out_lengths)])
        offsets = np.ceil(np.asarray(selected_trialdefinition(data))[:, 2] * resamplefs / samplerate)
        out.trialdefinition = np.stack([edges[:-1], edges[1:], offsets], axis=1)
        out.channel = selected_channel_labels(data)
        out.cfg = dict(getattr(data, "cfg", {}) or {})
        out.cfg["resampledata"] = new_cfg
        return out


def _model_run(data, rows, steps, out_lengths, ops):
    """The steps through a table of host functions (the tests' NumPy/SciPy model): ops["resample"](trial, taps_scaled, up,
    down), ops["downsample"](trial, skip), ops["fir"](trial, taps), each -> trial."""
    outs = []
    for x, n in zip(TrialSource(data, rows).host_trials(), out_lengths):
        x = np.array(x, dtype=np.float32)
        for step in steps:
            x = np.asarray(ops[step[0]](x, *step[1:]), dtype=np.float32)
        if x.shape[0] != n:
            raise ValueError(f"the model returned {x.shape[0]} samples, expected {n}")
        outs.append(x)
    return np.concatenate(outs, axis=0)


def _device_run(data, rows, steps, out_lengths):
    import torch
    from .. import backend
    backend.require_gpu()
    if data.data_dtype != np.float32:
        raise SPYTypeError(data.data_dtype, varname="data", expected="float32 data")
    source = TrialSource(data, rows)
    nchan, dev = source.nchan, source.dev
    lengths = [b - a for a, b in rows]
    starts = np.concatenate([[0], np.cumsum(out_lengths)]).astype(np.int64)
    res = torch.empty((int(starts[-1]), nchan), dtype=torch.float32, device=dev)
    result = ResultRows(starts, res)
    last = steps[-1]
    if last[0] == "resample":
        last_taps, up, down = last[1], last[2], last[3]
    else:                                           # the decimation, fused with the second filter pass if there is one
        last_taps, up, down = (steps[-2][1] if len(steps) > 1 else np.ones(1)), 1, last[1]
    last_taps = torch.as_tensor(np.ascontiguousarray(last_taps, dtype=np.float64), device=dev)
    first_taps = torch.as_tensor(np.ascontiguousarray(steps[0][1], dtype=np.float64), device=dev) if len(steps) > 1 else None
    for n, ks in equal_length_chunks(lengths, nchan, CHUNK_BYTES):
        m, nout = len(ks), int(out_lengths[ks[0]])
        x, _ = source.gather(ks, n)
        if first_taps is not None:
            # fir_same reports NaN trials; resampledata has no info["nan_trials"], so the flags are not read
            nan = torch.zeros(m, dtype=torch.int32, device=dev)
            x = backend.fir_same(x, torch.empty((m, n, nchan), dtype=torch.float32, device=dev), first_taps, nan)
        # output: straight into the result when the chunk's trials follow each other there
        direct = result.view(ks, nout)
        if direct is not None:
            backend.upfirdn(x, direct, last_taps, up, down)
        else:
            y = backend.upfirdn(x, torch.empty((m, nout, nchan), dtype=torch.float32, device=dev), last_taps, up, down)
            result.scatter(ks, nout, y)
    return res
