"""`spy.spike_psth`: peristimulus time histograms of SpikeData (syncopy/statistics/spike_psth.py, statistics/psth.py and
psth_cF / PSTH of statistics/compRoutines.py), on the device.

    spd = spy.synthdata.poisson_noise(nTrials=100, seed=1)
    tld = spy.spike_psth(spd, binsize=0.05, latency=[-0.1, 0.6], output="rate")
    tld.data                    # (nTrials * nBins, nColumns) float32, one column per (channel, unit) pair that fires
    tld.avg, tld.var            # (nBins, nColumns): spy.mean / spy.var over the trials

The spike table is uploaded once (`SpikeData.device_columns`) and read by the kernels of csrc/psth_kernel.h: which
(channel, unit) pairs occur, the row range of every (trial, bin) by binary search - the table is sorted by sample and the
time of a spike, (sample - start + onset) / samplerate in float64, does not decrease with it -, integer counts in LDS and
one store per element.  `spikecount` and `rate` are the reference's bits, `proportion` agrees to the order of a few
float64 operations ahead of the one rounding to float32.  `avg` and `var` go through the trial-moment kernels of spy.mean
and spy.var, the route spy.timelockanalysis takes.  Everything above the kernels (`_plan`) is NumPy and needs no GPU;
there is no CPU path for the histogram itself.

The reference's code is followed, not its docstrings: 'rice' / 'sqrt' take the mean trial length in SAMPLES and give
that many EDGES (one bin less); the NaN mask of psth.py:133-155 is kept with both "mask all" branches and with index 0
meaning "no mask".

Deviations from the reference, on purpose:
  * a spike on channel c, unit u counts in column (c, u).  The reference passes raw channel numbers to histogram2d with
    the channel bins arange(k + 1), k = number of distinct channels in that trial, so whenever a trial's channels are not
    exactly 0 .. k-1 it counts spikes into the wrong column (channels 1, 2, 2 with the columns (0,0), (1,0), (2,0) give
    [0, 0, 3], the evident intent is [0, 1, 2]).  The two agree when every trial holds a selected spike on each channel
    0 .. C-1;
  * SpikeData sorts its rows by sample at construction (the reference never sorts and then cuts arbitrary trials);
  * the time window is the `latency` argument: a "latency" key in `select` is refused;
  * `.spike` containers are neither saved nor loaded;
  * a selection that leaves no spike at all raises (there: an array without columns);
  * a histogram of one bin gets the samplerate 1 / bin width (there: NaN, the mean of no midpoint differences).
"""
import types

import numpy as np

from ..datatype import TimeLockData
from ..datatype.spike_data import SpikeData
from ..shared.errors import SPYInfo, SPYTypeError, SPYValueError
from ..shared.trial_chunks import applied_selection, reject_unknown_kwargs

__all__ = ["spike_psth"]

available_outputs = ["rate", "spikecount", "proportion"]
available_latencies = ["maxperiod", "minperiod", "prestim", "poststim"]
# bytes of histogram held on the device at once
CHUNK_BYTES = 512 << 20
# entries of the (channel, unit) tables (MAX_TABLE of csrc/psth.hip)
MAX_TABLE = 1 << 24


def rice_rule(nSamples):
    return int(2 * pow(nSamples, 1 / 3))


def sqrt_rule(nSamples):
    return int(np.ceil(np.sqrt(nSamples)))


available_binsizes = {"rice": rice_rule, "sqrt": sqrt_rule}


def spike_psth(data, binsize="rice", output="rate", latency="maxperiod", vartriallen=True, keeptrials=True, select=None,
               **kwargs):
    """Peristimulus time histogram.

    binsize     : bin width in seconds, or 'rice' / 'sqrt': that rule's number of bin EDGES for the mean trial length
    output      : 'rate' (spikes per second), 'spikecount', or 'proportion' (area under every histogram 1)
    latency     : [t0, t1] in seconds, or 'maxperiod' (default), 'minperiod', 'prestim', 'poststim'
    vartriallen : True takes every trial and leaves NaN in the bins a trial does not reach; False keeps only the trials
                  that cover the whole window
    keeptrials  : False leaves `data` None and the trial definition at one row; `avg` and `var` are filled either way
    select      : in-place selection {"trials", "channel", "unit"}

    Returns TimeLockData with the histograms of the trials stacked along time and one channel "channel{c}_unit{u}" per
    pair that occurs.  `chan_per_worker` / `parallel` are accepted and ignored."""
    if not isinstance(data, SpikeData):
        raise SPYTypeError(data, varname="data", expected="Syncopy SpikeData object")
    if data.data is None or data.trialdefinition is None or data.samplerate is None:
        raise SPYValueError("non-empty Syncopy data object with a samplerate", varname="data", actual="empty object")
    if not isinstance(vartriallen, bool):
        raise SPYTypeError(vartriallen, varname="vartriallen", expected="bool")
    if not isinstance(keeptrials, bool):
        raise SPYTypeError(keeptrials, varname="keeptrials", expected="bool")
    new_cfg = dict(binsize=binsize, output=output, latency=latency, vartriallen=vartriallen, keeptrials=keeptrials)
    reject_unknown_kwargs(kwargs, new_cfg)
    if select is not None:
        new_cfg["select"] = select

    with applied_selection(data, select):
        plan = _plan(data, binsize, output, latency, vartriallen, presence=_device_presence(data))
        if not vartriallen:
            SPYInfo(f"Discarded {plan.numDiscard} trials which did not fit into latency window")
        tld = TimeLockData(None, samplerate=plan.out_samplerate)
        tld.trialdefinition = plan.trialdefinition if keeptrials else plan.trialdefinition[[0], :]
        tld.channel = np.array(plan.labels)
        tld.cfg = dict(getattr(data, "cfg", {}) or {})
        tld.cfg["spike_psth"] = new_cfg
        tld.info = dict(plan.log_dict)
        tld.log = "".join(f"{k} = {v}\n" for k, v in plan.log_dict.items())
        _device_run(data, plan, tld, keeptrials)
        return tld


# ---- everything above the kernels, in NumPy ---------------------------------------------------------------------------
def analysis_window(intervals, latency):
    """[t0, t1] in seconds for the trials' [start, end] times `intervals` (shared/latency.py: get_analysis_window)"""
    starts, ends = intervals[:, 0], intervals[:, 1]
    if isinstance(latency, str):
        if latency not in available_latencies:
            raise SPYValueError(f"one of {available_latencies}", varname="latency", actual=latency)
        if latency == "minperiod":
            window = [np.max(starts), np.min(ends)]
            if window[0] > window[1]:
                raise SPYValueError("overlapping trials", "latency", f"{latency} - no common time window for all trials")
        elif latency == "maxperiod":
            window = [np.min(starts), np.max(ends)]
        elif latency == "prestim":
            if not np.any(starts < 0):
                raise SPYValueError("pre-stimulus recordings", "latency", "no pre-stimulus (t < 0) events")
            window = [np.min(starts), 0]
        else:
            if not np.any(ends > 0):
                raise SPYValueError("post-stimulus recordings", "latency", "no post-stimulus (t > 0) events")
            window = [0, np.max(ends)]
        return window
    try:
        lat = np.array(latency, dtype=float)
    except (TypeError, ValueError):
        raise SPYTypeError(latency, varname="latency", expected="array like [start, end]") from None
    if lat.shape != (2,) or np.any(np.isnan(lat)):
        raise SPYValueError("array like [start, end]", varname="latency", actual=str(latency))
    if lat[0] > ends.max():
        raise SPYValueError(f"start of latency window < {ends.max()}s", "latency[0]", lat[0])
    if lat[1] < starts.min():
        raise SPYValueError(f"end of latency window > {starts.min()}s", "latency[1]", lat[1])
    if lat[0] > lat[1]:
        raise SPYValueError("start < end latency window", "latency", f"start={lat[0]}, end={lat[1]}")
    return [float(lat[0]), float(lat[1])]


def bin_edges(binsize, window, av_trl_size):
    """the float64 bin edges of spike_psth.py:180-190"""
    if isinstance(binsize, str):
        if binsize not in available_binsizes:
            raise SPYValueError(f"one of {list(available_binsizes)}", varname="binsize", actual=binsize)
        n = available_binsizes[binsize](av_trl_size)
        if n < 2:
            raise SPYValueError("trials long enough for two bin edges", varname="binsize", actual=f"{binsize}: {n}")
        return np.linspace(*window, n)
    if isinstance(binsize, bool) or not isinstance(binsize, (int, float, np.integer, np.floating)):
        raise SPYTypeError(binsize, varname="binsize", expected="scalar or one of 'rice', 'sqrt'")
    width = float(np.diff(window).squeeze())
    if not np.isfinite(binsize) or binsize < 0 or binsize > width:
        raise SPYValueError(f"value to be greater or equals 0 and less or equals {width}", varname="binsize",
                            actual=str(binsize))
    if binsize == 0:
        raise SPYValueError("a bin width that gives at least one bin", varname="binsize", actual=str(binsize))
    return np.arange(window[0], window[1] + binsize, binsize)


def valid_bins(edges, start, end, onset, samplerate):
    """[lo, hi): the bins of one trial that psth.py:133-155 leaves unmasked"""
    nbins = len(edges) - 1
    trl_start_reltime = onset / samplerate
    trl_end_reltime = (end - start + onset) / samplerate
    if np.all(edges < trl_start_reltime):
        min_idx = nbins
    else:
        min_idx = int(np.argmin(edges < trl_start_reltime))
    if np.all(edges > trl_end_reltime):
        min_idx = nbins
        max_idx = 0
    else:
        max_idx = int(np.argmin(edges <= trl_end_reltime))
    return min(min_idx, nbins), (min(max_idx, nbins) if max_idx != 0 else nbins)


def valid_bins_all(edges, start, end, onset, samplerate):
    """valid_bins for arrays of trials at once, as (T, 2) int32: for ascending edges the first index at which a comparison
    fails is the number of edges for which it holds"""
    edges = np.asarray(edges, dtype=np.float64)
    nbins = len(edges) - 1
    t0 = np.asarray(onset, dtype=np.float64) / samplerate
    t1 = (np.asarray(end, dtype=np.float64) - np.asarray(start, dtype=np.float64) + onset) / samplerate
    lo = np.minimum(np.searchsorted(edges, t0, side="left"), nbins)
    upto = np.searchsorted(edges, t1, side="right")               # edges <= end; all of them: index 0, no tail mask
    hi = np.where(upto == len(edges), nbins, np.minimum(upto, nbins))
    behind = edges[0] > t1
    return np.stack([np.where(behind, nbins, lo), np.where(behind, nbins, hi)], axis=1).astype(np.int32)


def column_tables(flags):
    """from the (C, U) presence table: the columns (sorted (channel, unit) pairs), lut[channel * U + unit] -> column or
    -1, unit_k[unit] -> dense index of the units that have a column or -1, col_k[column] -> its unit's dense index, and
    the number of such units"""
    C, U = flags.shape
    columns = np.argwhere(flags != 0).astype(np.int64)      # sorted by channel, then unit
    lut = np.full(C * U, -1, dtype=np.int32)
    lut[columns[:, 0] * U + columns[:, 1]] = np.arange(columns.shape[0], dtype=np.int32)
    units = np.unique(columns[:, 1])
    unit_k = np.full(U, -1, dtype=np.int32)
    unit_k[units] = np.arange(units.size, dtype=np.int32)
    return columns, lut, unit_k, np.ascontiguousarray(unit_k[columns[:, 1]]), int(units.size)


def _host_presence(pre):
    """flags[channel * U + unit] = 1 for the selected spikes of the selected trials, in NumPy (what psth_presence_kernel
    computes on the device)"""
    flags = np.zeros(pre.C * pre.U, dtype=np.uint8)
    chan, unit = pre.table[:, 1], pre.table[:, 2]
    for a, b in set(zip(pre.row_lo.tolist(), pre.row_hi.tolist())):
        c, u = chan[a:b], unit[a:b]
        ok = pre.chan_ok[c].astype(bool) & pre.unit_ok[u].astype(bool)
        flags[c[ok] * pre.U + u[ok]] = 1
    return flags


def _plan(data, binsize, output, latency, vartriallen, presence=None):
    """All a spike_psth call decides ahead of the kernels, from `data` and its in-place selection: the window, the kept
    trials, the float64 edges, the columns and their look-up table, per trial the row range, start, onset and valid
    bins, and the metadata of the result.  `presence(pre)` -> uint8 flags[channel * U + unit] of the pairs that occur
    (None: NumPy)."""
    if output not in available_outputs:
        raise SPYValueError(f"one of {available_outputs}", "output", output)
    if isinstance(binsize, str) and binsize not in available_binsizes:
        raise SPYValueError(f"one of {list(available_binsizes)}", "binsize", binsize)
    sel = data.selection
    srate = float(data.samplerate)
    trl_all = data.trialdefinition
    trial_ids = list(range(trl_all.shape[0])) if sel is None else list(sel.trial_ids)
    if len(trial_ids) < 1:
        raise SPYValueError("at least 1 trial", varname="data", actual="got 0 trials")
    intervals = data.trialintervals[trial_ids]
    window = analysis_window(intervals, latency)

    numDiscard = 0
    if not vartriallen:                                   # shared/latency.py: create_trial_selection
        fits = (intervals[:, 0] <= window[0]) & (intervals[:, 1] >= window[1])
        kept = [t for t, ok in zip(trial_ids, fits) if ok]
        if not kept:
            raise SPYValueError("at least one trial covering the latency window", varname="latency/vartriallen",
                                actual="no trial that completely covers the latency window")
        numDiscard = len(trial_ids) - len(kept)
        trial_ids = kept
    trl = trl_all[trial_ids]
    if np.any(trl[:, 2] != np.rint(trl[:, 2])):
        raise SPYValueError("integer trigger offsets (in samples)", varname="trialdefinition", actual="fractional offsets")
    start, end, onset = (trl[:, k].astype(np.int64) for k in range(3))

    av_trl_size = (end - start).sum() / len(trial_ids)
    edges = np.asarray(bin_edges(binsize, window, av_trl_size), dtype=np.float64)
    nbins = len(edges) - 1
    if nbins < 1:
        raise SPYValueError("a window that holds at least one bin", varname="binsize", actual=str(binsize))

    C, U = int(data.channel_idx.max()) + 1, int(data.unit_idx.max()) + 1
    if C * U > MAX_TABLE:
        raise SPYValueError(f"(largest channel number + 1) x (largest unit number + 1) <= {MAX_TABLE}", varname="data",
                            actual=f"{C} x {U}")
    chan_ok, unit_ok = np.zeros(C, dtype=np.uint8), np.zeros(U, dtype=np.uint8)
    chan_ok[data.channel_idx if sel is None else sel.channel] = 1
    unit_ok[data.unit_idx if sel is None else sel.unit] = 1
    rows = data.trial_rows[trial_ids]
    pre = types.SimpleNamespace(table=data.data, row_lo=np.ascontiguousarray(rows[:, 0]),
                                row_hi=np.ascontiguousarray(rows[:, 1]), chan_ok=chan_ok, unit_ok=unit_ok, C=C, U=U)
    flags = np.asarray((presence or _host_presence)(pre), dtype=np.uint8).reshape(C, U)
    columns, lut, unit_k, col_k, nk = column_tables(flags)
    ncols = columns.shape[0]
    if ncols == 0:
        raise SPYValueError("at least one spike in the selected trials, channels and units", varname="select",
                            actual="no spike")

    if np.any(np.diff(edges) <= 0):
        raise SPYValueError("ascending bin edges", varname="binsize", actual=str(binsize))
    lohi = valid_bins_all(edges, trl[:, 0], trl[:, 1], trl[:, 2], srate)
    scale = float(1 / np.diff(edges)[0]) if output == "rate" else 1.0

    # PSTH.process_metadata
    mid = (edges[:-1] + edges[1:]) / 2
    out_srate = float(1 / np.diff(mid).mean()) if nbins > 1 else float(1 / np.diff(edges)[0])
    out_trl = np.zeros((len(trial_ids), 3))
    bounds = np.arange(0, len(trial_ids) * nbins + 1, nbins)
    out_trl[:, 0], out_trl[:, 1] = bounds[:-1], bounds[1:]
    out_trl[:, 2] = np.rint(mid[0] * out_srate)
    log_dict = {"bins": edges, "binsize": binsize, "latency": latency, "output": output, "vartriallen": vartriallen,
                "numDiscard": numDiscard}
    return types.SimpleNamespace(
        window=window, trial_ids=trial_ids, numDiscard=numDiscard, edges=edges, nbins=nbins, columns=columns, ncols=ncols,
        labels=[f"channel{c}_unit{u}" for c, u in columns], lut=lut, C=C, U=U, chan_ok=chan_ok, unit_ok=unit_ok,
        unit_k=unit_k, col_k=col_k, nk=nk, row_lo=pre.row_lo, row_hi=pre.row_hi,
        start=start, onset=onset, lohi=np.ascontiguousarray(lohi), scale=scale, output=output, samplerate=srate,
        out_samplerate=out_srate, trialdefinition=out_trl, log_dict=log_dict)


# ---- the device work ------------------------------------------------------------------------------------------------
def _device_presence(data):
    """`presence` of _plan through psth_presence_kernel on the resident table (no GPU: the package's usual error)"""
    def presence(pre):
        import torch
        from .. import backend
        _, chan, unit = data.device_columns()
        up = lambda a: torch.from_numpy(a).to(chan.device)      # noqa: E731
        flags = backend.psth_presence(chan, unit, up(pre.row_lo), up(pre.row_hi), int((pre.row_hi - pre.row_lo).max()),
                                      up(pre.chan_ok), up(pre.unit_ok))
        return flags.cpu().numpy()
    return presence


def _device_run(data, plan, tld, keeptrials):
    import torch
    from .. import backend
    backend.require_gpu()
    sample, chan, unit = data.device_columns()
    dev = sample.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    T, nbins, ncols = len(plan.trial_ids), plan.nbins, plan.ncols
    row_lo, row_hi, start, onset = up(plan.row_lo), up(plan.row_hi), up(plan.start), up(plan.onset)
    lohi, lut, edges = up(plan.lohi), up(plan.lut), up(plan.edges)
    prop = (up(plan.unit_k), up(plan.col_k), plan.nk) if plan.output == "proportion" else None
    per = max(1, CHUNK_BYTES // (nbins * ncols * 4))
    chunks = [(a, min(a + per, T)) for a in range(0, T, per)]

    def histogram(a, b):
        """the trials [a, b) of the result as an (b - a, nbins, ncols) float32 tensor"""
        rows = backend.psth_bin_rows(sample, row_lo[a:b], row_hi[a:b], start[a:b], onset[a:b], edges, plan.samplerate)
        out = backend.psth_count(chan, unit, rows, lut, plan.C, plan.U, lohi[a:b], ncols, plan.scale)
        if prop is not None:
            backend.psth_proportion(chan, unit, row_lo[a:b], row_hi[a:b], rows, lut, plan.C, plan.U, *prop, edges, out)
        return out

    host = np.empty((T * nbins, ncols), dtype=np.float32) if keeptrials and len(chunks) > 1 else None
    acc = torch.zeros((nbins, ncols), dtype=torch.float32, device=dev)
    kept = None
    for a, b in chunks:
        x = histogram(a, b)
        backend.trial_sum(x, acc)
        if host is not None:
            host[a * nbins:b * nbins] = backend.to_host(x.view(-1, ncols))
        if len(chunks) == 1:
            kept = x                                    # one chunk: pass 2 needs no second histogram
    mean = backend.trial_sum_finalize(acc, T)
    sq = torch.zeros((nbins, ncols), dtype=torch.float32, device=dev)
    for a, b in chunks:
        backend.trial_sqdev(kept if kept is not None else histogram(a, b), mean, sq)
    tld.avg = backend.to_host(mean)
    tld.var = backend.to_host(backend.trial_var_finalize(sq, T, torch.float32, False))
    if keeptrials:
        tld.data = host if host is not None else backend.to_host(kept.view(-1, ncols))
