"""NumPy model of spy.var / spy.std / spy.median / spy.itc (syncopy statistics/summary_stats.py:156-205, 321-486 and
statistics/compRoutines.py:22-141), written from the contract: the operations in the `routine_classes` shape that
`syncopy_amd.statistics.summary_stats` takes with compute_method="sequential"."""
import numpy as np


def trial_mean(trials):
    """`out += trl` over the trials in the data's dtype, then one division (summary_stats.py:408-428)."""
    out = np.zeros(trials[0].shape, dtype=trials[0].dtype)
    for trl in trials:
        out += trl
    out /= len(trials)
    return out


def trial_var(trials):
    """Two passes in the data's dtype: the trial mean, then `out += |trl - mean|**2` in trial order, `out /= T`.
    NaNs are not skipped."""
    average = trial_mean(trials)
    out = np.zeros(trials[0].shape, dtype=trials[0].dtype)
    for trl in trials:
        out += np.abs(trl - average) ** 2
    out /= len(trials)
    return out


def trial_std(trials):
    return np.sqrt(trial_var(trials))


def itc(trials, taper_axis):
    """|mean over tapers of (sum over trials of z / |z|) / T| as float32; the taper axis is kept with length 1."""
    out = np.zeros(trials[0].shape, dtype=trials[0].dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for trl in trials:
            out += trl / np.abs(trl)
    out /= len(trials)
    return np.abs(np.mean(out, axis=taper_axis, keepdims=True))


def _in_dtype(res, trl):
    """npstats_cF allocates its output in the trial's dtype (compRoutines.py:56): real results of complex data are
    stored with imaginary part 0."""
    return np.asarray(res).astype(trl.dtype)


def _quiet(fn, trl, axis):
    """all-NaN slices give NaN with a RuntimeWarning, which the reference's users see and the tests do not need"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return _in_dtype(fn(trl, axis=axis, keepdims=True), trl)


def axis_var(trl, axis):
    return _quiet(np.nanvar, trl, axis)


def axis_std(trl, axis):
    return _quiet(np.nanstd, trl, axis)


def axis_median(trl, axis):
    return _quiet(np.nanmedian, trl, axis)


def axis_mean(trl, axis):
    return np.nanmean(trl, axis=axis, keepdims=True)


STATS_OPS = {"trial_mean": trial_mean, "trial_var": trial_var, "trial_std": trial_std, "itc": itc,
             "axis_mean": axis_mean, "axis_var": axis_var, "axis_std": axis_std, "axis_median": axis_median}
