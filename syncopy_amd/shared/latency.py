"""The latency window of a front end and the trials that cover it (syncopy/shared/latency.py: get_analysis_window :17-96,
create_trial_selection :99-166).  Both respect an in-place selection on `data`.  NumPy only."""
import numpy as np

from .errors import SPYValueError

available_latencies = ["maxperiod", "minperiod", "prestim", "poststim"]


def _selected_intervals(data):
    """(ids, starts, ends): the selected trials and their first and last sample time in seconds"""
    if data.selection is not None:
        trl = np.asarray(data.selection.trialdefinition, dtype=float)
        n = trl[:, 1] - trl[:, 0]
        iv = np.stack([trl[:, 2], trl[:, 2] + n - 1], axis=1) / data.samplerate
        ids = np.array(data.selection.trial_ids, dtype=np.int64)
    else:
        iv = data.trialintervals
        ids = np.arange(iv.shape[0])
    return ids, iv[:, 0], iv[:, 1]


def get_analysis_window(data, latency):
    """[start, end] in seconds of `latency`: 'maxperiod', 'minperiod', 'prestim', 'poststim' or [start, end]"""
    _, trl_starts, trl_ends = _selected_intervals(data)
    if isinstance(latency, str):
        if latency not in available_latencies:
            raise SPYValueError(f"one of {available_latencies}", varname="latency", actual=latency)
        if latency == "minperiod":
            window = [np.max(trl_starts), np.min(trl_ends)]
            if window[0] > window[1]:
                raise SPYValueError("overlapping trials", "latency", f"{latency} - no common time window for all trials")
        elif latency == "maxperiod":
            window = [np.min(trl_starts), np.max(trl_ends)]
        elif latency == "prestim":
            if not np.any(trl_starts < 0):
                raise SPYValueError("pre-stimulus recordings", "latency", "no pre-stimulus (t < 0) events")
            window = [np.min(trl_starts), 0]
        else:
            if not np.any(trl_ends > 0):
                raise SPYValueError("post-stimulus recordings", "latency", "no post-stimulus (t > 0) events")
            window = [0, np.max(trl_ends)]
        return [float(window[0]), float(window[1])]
    try:
        lat = np.array(latency, dtype=float)
    except (TypeError, ValueError):
        lat = np.empty(0)
    if lat.shape != (2,) or np.isnan(lat).any():
        raise SPYValueError("[start, end] in seconds", varname="latency", actual=str(latency))
    if lat[0] > trl_ends.max():
        raise SPYValueError(f"start of latency window < {trl_ends.max()}s", "latency[0]", lat[0])
    if lat[1] < trl_starts.min():
        raise SPYValueError(f"end of latency window > {trl_starts.min()}s", "latency[1]", lat[1])
    if lat[0] > lat[1]:
        raise SPYValueError("start < end latency window", "latency", f"start={lat[0]}, end={lat[1]}")
    return [float(lat[0]), float(lat[1])]


def create_trial_selection(data, window):
    """(select, numDiscard): a `select` dictionary (the existing one amended, or a new one) that keeps only the trials
    which cover `window` completely, in their selection order, and how many it discards"""
    ids, trl_starts, trl_ends = _selected_intervals(data)
    fit = ids[(trl_starts <= window[0]) & (trl_ends >= window[1])]
    if fit.size == 0:
        raise SPYValueError("at least one trial covering the latency window", varname="latency/vartriallen",
                            actual="no trial that completely covers the latency window")
    if data.selection is None:
        return {"trials": fit}, len(ids) - len(fit)
    keep = set(fit.tolist())                # (a trial selected twice has one window: it stays or goes as a whole)
    fit = np.array([t for t in data.selection.trial_ids if t in keep], dtype=np.int64)
    select = dict(data.selection.select)
    select["trials"] = fit
    return select, len(ids) - len(fit)
