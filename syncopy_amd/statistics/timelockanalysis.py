"""`spy.timelockanalysis`: trial average, variance and channel covariance of AnalogData (syncopy/statistics/
timelockanalysis.py with cov_cF / Covariance of statistics/compRoutines.py), on the device.

    tld = spy.timelockanalysis(adata, latency=[-0.2, 0.5], covariance=True)
    tld.avg, tld.var            # (nSamples, nChannels): spy.mean / spy.var over the trials of the window
    tld.cov                     # (nChannels, nChannels): trial average of np.cov(trial, rowvar=False)

`latency` is applied on top of an existing selection of trials and channels; the cut trials are stacked along time in
`tld.data`.  `avg` and `var` go through the kernels of spy.mean / spy.var (sequential float32 sum over the trials, two-pass
variance), `cov` through the fp64 matrix-core kernel of csrc/cov.hip: np.cov per trial in float64, rounded to float32
once, then - unless keeptrials - the engine's trial average, a sequential float32 sum and one division.  The trials pass
through the device in chunks of at most CHUNK_BYTES, by the routes of shared/trial_chunks.py, and there is no CPU path;
`compute_method="sequential"` with `routine_classes` swaps in a table of NumPy functions (trial_mean, trial_var, cov) for
the tests.

Deviations from the reference, on purpose:
  * n - ddof <= 0 raises SPYValueError (there NumPy warns and the result is inf / NaN);
  * the reference's docstring has the meaning of `keeptrials` inverted; this follows its code: True keeps the per-trial
    matrices;
  * `.timelock` containers are neither saved nor loaded;
  * float32 input only, and time must be the first axis, as in spy.preprocessing.
"""
import numpy as np

from ..datatype import TimeLockData, selected_channel_labels, selected_channels, selected_trialdefinition, trial_rows
from ..shared.errors import SPYTypeError, SPYValueError
from ..shared.trial_chunks import (TrialSource, applied_selection, check_analog_input, equal_length_chunks,
                                   reject_unknown_kwargs)

__all__ = ["timelockanalysis"]

# bytes of trials held on the device at once
CHUNK_BYTES = 512 << 20


def timelockanalysis(data, latency="maxperiod", covariance=False, ddof=None, trials="all", keeptrials=False, select=None,
                     compute_method=None, routine_classes=None, **kwargs):
    """Average, variance and channel covariance of AnalogData across trials.

    latency    : [t0, t1] in seconds, or 'maxperiod' (default), 'minperiod', 'prestim', 'poststim'
    covariance : True also computes the covariance between the channels
    ddof       : degrees of freedom of the covariance: the sum is divided by N - ddof; None is N - 1
    trials     : 'all' or a sequence of trial indices; not together with a trial selection
    keeptrials : True leaves the covariance of every trial in `cov`, False their average over the trials
    select     : in-place selection {"trials", "channel"}; its latency is replaced by `latency`

    Returns TimeLockData: `data` holds the selected trials cut to the window and stacked along time, `avg` and `var` are
    (nSamples, nChannels), `cov` is None, (nChannels, nChannels) or (nTrials, nChannels, nChannels), squeezed.  All cut
    trials need the same length.  `chan_per_worker` / `parallel` are accepted and ignored."""
    check_analog_input(data)
    if data.data_dtype != np.float32:
        raise SPYTypeError(data.data_dtype, varname="data", expected="float32 data")
    if ddof is not None and (not isinstance(ddof, int) or isinstance(ddof, bool) or ddof < 0):
        raise SPYValueError("positive integer value", varname="ddof", actual=str(ddof))
    if not isinstance(covariance, bool):
        raise SPYTypeError(covariance, varname="covariance", expected="bool")
    if not isinstance(keeptrials, bool):
        raise SPYTypeError(keeptrials, varname="keeptrials", expected="bool")
    new_cfg = dict(latency=latency, covariance=covariance, ddof=ddof, trials=trials, keeptrials=keeptrials)
    reject_unknown_kwargs(kwargs, new_cfg)
    if select is not None:
        new_cfg["select"] = select
    all_trials = isinstance(trials, str) and trials == "all"

    with applied_selection(data, select):
        sel = {} if data.selection is None else dict(data.selection.select)
        if not all_trials:
            if sel.get("trials") is not None:
                raise SPYValueError("either `trials != 'all'` or selection", varname="trials",
                                    actual="trial keyword and trial selection")
            sel["trials"] = trials
        sel["latency"] = latency
        data.selectdata(sel)

        rows = trial_rows(data)
        if len(rows) < 1:
            raise SPYValueError("at least 1 trial", varname="data", actual="got 0 trials")
        lengths = [b - a for a, b in rows]
        chans = selected_channels(data)
        nchan = int(data.data_shape[1]) if chans is None else len(chans)
        for n in lengths:
            if n != lengths[0]:                 # what spy.mean / spy.var over the trials raise
                raise SPYValueError("all trials to have the same shape", varname="in_data",
                                    actual=f"found trials of different shape: {(lengths[0], nchan)} and {(n, nchan)}")
        n = int(lengths[0])
        if n < 1:
            raise SPYValueError("a latency window that holds samples", varname="latency", actual=str(latency))
        dof = 1 if ddof is None else ddof
        if covariance and n - dof <= 0:
            raise SPYValueError(f"fewer degrees of freedom than the {n} samples of a trial", varname="ddof", actual=str(ddof))

        tld = TimeLockData(None, samplerate=data.samplerate, dimord=data.dimord)
        tld.trialdefinition = selected_trialdefinition(data)
        tld.channel = selected_channel_labels(data)
        tld.cfg = dict(getattr(data, "cfg", {}) or {})
        tld.cfg["timelockanalysis"] = new_cfg
        if compute_method in (None, "hip"):
            _device_run(data, tld, rows, n, covariance, dof, keeptrials)
        else:
            _model_run(data, tld, rows, covariance, ddof, keeptrials, routine_classes)
        return tld


def _model_run(data, tld, rows, covariance, ddof, keeptrials, ops):
    """Through a table of host functions (the tests' NumPy model): ops["trial_mean"](trials), ops["trial_var"](trials),
    ops["cov"](trial, ddof) -> float32 (nchan, nchan)."""
    stacked = np.asarray(TrialSource(data, rows).host_stack(), dtype=np.float32)
    n = rows[0][1] - rows[0][0]
    trials = [stacked[k * n:(k + 1) * n] for k in range(len(rows))]
    tld.data = stacked
    tld.avg = np.asarray(ops["trial_mean"](trials), dtype=np.float32)
    tld.var = np.asarray(ops["trial_var"](trials), dtype=np.float32)
    if covariance:
        per = [np.asarray(ops["cov"](x, ddof), dtype=np.float32) for x in trials]
        cov = np.stack(per) if keeptrials else np.asarray(ops["trial_mean"](per), dtype=np.float32)
        tld.cov = cov.squeeze()


def _device_run(data, tld, rows, n, covariance, ddof, keeptrials):
    import torch
    from .. import backend
    backend.require_gpu()
    source = TrialSource(data, rows)
    nchan, dev = source.nchan, source.dev
    T = len(rows)
    chunks = [ks for _, ks in equal_length_chunks([n] * T, nchan, CHUNK_BYTES)]     # runs of consecutive trials

    # pass 1: the trial sum, and the covariance of every trial while it is on the device
    acc = torch.zeros((n, nchan), dtype=torch.float32, device=dev)
    cov = None
    if covariance:
        cov = (torch.empty if keeptrials else torch.zeros)((T, nchan, nchan) if keeptrials else (nchan, nchan),
                                                          dtype=torch.float32, device=dev)
    kept = None
    for ks in chunks:
        x, _ = source.gather(ks, n)
        backend.trial_sum(x, acc)
        if covariance and keeptrials:
            backend.cov(x, ddof, out=cov[ks[0]:ks[-1] + 1])
        elif covariance:
            backend.trial_sum(backend.cov(x, ddof), cov)
        if len(chunks) == 1:
            kept = x                                # one chunk: pass 2 needs no second upload
    mean = backend.trial_sum_finalize(acc, T)
    if covariance and not keeptrials:
        backend.trial_sum_finalize(cov, T)
    # pass 2: the squared deviations from the trial mean
    sq = torch.zeros((n, nchan), dtype=torch.float32, device=dev)
    for ks in chunks:
        backend.trial_sqdev(kept if kept is not None else source.gather(ks, n)[0], mean, sq)
    kept = None
    tld.avg = backend.to_host(mean)
    tld.var = backend.to_host(backend.trial_var_finalize(sq, T, torch.float32, False))
    if covariance:
        tld.cov = backend.to_host(cov).squeeze()

    if data._data is not None:
        tld.data = source.host_stack()
    else:                                           # the input lives on the device only: fetch the rows when asked for
        tld.set_pending(source.fetch_rows, (T * n, nchan), np.float32)
