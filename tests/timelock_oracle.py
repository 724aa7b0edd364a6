"""NumPy model of spy.timelockanalysis (syncopy statistics/timelockanalysis.py and cov_cF of statistics/compRoutines.py),
written from the contract: the operations in the `routine_classes` shape that `syncopy_amd.statistics.timelockanalysis`
takes with compute_method="sequential".  `avg` and `var` are the trial statistics of stats_oracle."""
import numpy as np

from stats_oracle import STATS_OPS


def cov(trial, ddof=None):
    """np.cov over the channels of one (time x channel) trial - float64 inside - stored as float32 (cov_cF hands the
    float64 matrix to a float32 dataset)."""
    return np.atleast_2d(np.cov(trial, ddof=ddof, rowvar=False)).astype(np.float32)


def cov_average(per_trial):
    """the engine's trial average of the per-trial matrices: a sequential float32 sum over the trials, one division"""
    return STATS_OPS["trial_mean"]([np.asarray(c, dtype=np.float32) for c in per_trial])


TIMELOCK_OPS = {"trial_mean": STATS_OPS["trial_mean"], "trial_var": STATS_OPS["trial_var"], "cov": cov}
