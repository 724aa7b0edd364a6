"""NumPy model of spy.spike_psth, written from the rules of the feature's specification (not from the reference's
function): counting by searchsorted per column, explicit loops, everything in float64 and one rounding to float32.

A spike on channel c, unit u counts in column (c, u) - the intent of the reference's histogram2d call, and what it
computes whenever every trial holds a spike on each channel 0 .. C-1 (the recorded fixtures are chosen that way).
"""
import numpy as np


def valid_range(edges, start, end, onset, samplerate):
    """[lo, hi): the bins that stay unmasked.  The head of the histogram is NaN up to the first edge that is not before
    the trial's first sample time, the tail from the first edge behind the time one sample past its last; no edge
    behind it: no tail mask; all edges before the trial, or all behind it: everything is masked."""
    nbins = len(edges) - 1
    t_first = onset / samplerate
    t_end = (end - start + onset) / samplerate
    lo = nbins
    for i, e in enumerate(edges):
        if not e < t_first:
            lo = i
            break
    if all(e > t_end for e in edges):
        return nbins, nbins
    hi = nbins
    for i, e in enumerate(edges):
        if not e <= t_end:
            hi = i if i != 0 else nbins
            break
    return min(lo, nbins), min(hi, nbins)


def trial_psth(spikes, start, end, onset, columns, edges, output, samplerate):
    """(nbins, ncols) float32 for the (already selected) spikes `spikes` (n, 3) of one trial, sorted by sample"""
    edges = np.asarray(edges, dtype=np.float64)
    nbins = len(edges) - 1
    spikes = np.asarray(spikes).reshape(-1, 3)
    t = (spikes[:, 0] - start + onset) / samplerate
    counts = np.zeros((nbins, len(columns)), dtype=np.float64)
    for j, (c, u) in enumerate(columns):
        tt = np.sort(t[(spikes[:, 1] == c) & (spikes[:, 2] == u)])
        first = np.searchsorted(tt, edges, side="left")           # spikes before every edge
        first[-1] = np.searchsorted(tt, edges[-1], side="right")  # the last bin is closed on the right
        for b in range(nbins):
            counts[b, j] = first[b + 1] - first[b]
    lo, hi = valid_range(edges, start, end, onset, samplerate)
    res = counts.copy()
    if output == "rate":
        res = counts * (1 / np.diff(edges)[0])
    elif output == "proportion":
        dt = np.diff(edges)
        for j, (c, u) in enumerate(columns):
            mine = spikes[:, 2] == u
            if not mine.any():
                res[:, j] = 0.0                                   # the unit does not occur in the trial
                continue
            S = int(np.sum((t[mine] >= edges[0]) & (t[mine] <= edges[-1])))
            with np.errstate(invalid="ignore", divide="ignore"):
                for b in range(nbins):
                    res[b, j] = counts[b, j] / dt[b] / np.float64(S)     # 0 / 0: unit present, nothing in the window
    res[:lo] = np.nan
    res[hi:] = np.nan
    if output == "proportion":
        for j in range(len(columns)):
            total = 0.0
            for b in range(nbins):
                if not np.isnan(res[b, j]):
                    total += res[b, j]
            res[:, j] = res[:, j] / (total if total != 0 else 1.0)
    return res.astype(np.float32)


def selected(table, lo, hi, channels=None, units=None):
    """rows [lo, hi) of the table that pass the channel / unit selection (None: all)"""
    blk = table[lo:hi]
    ok = np.ones(len(blk), dtype=bool)
    if channels is not None:
        ok &= np.isin(blk[:, 1], list(channels))
    if units is not None:
        ok &= np.isin(blk[:, 2], list(units))
    return blk[ok]


def psth(table, trialdefinition, trial_ids, edges, output, samplerate, channels=None, units=None):
    """(columns (ncols, 2), result (len(trial_ids) * nbins, ncols) float32) for the sorted table and the trials
    `trial_ids` (any order, repeats allowed) of `trialdefinition` [start, end, onset]"""
    table = np.asarray(table, dtype=np.int64)
    trl = np.asarray(trialdefinition, dtype=np.float64)
    per = []
    for t in trial_ids:
        a, b = np.searchsorted(table[:, 0], [int(trl[t, 0]), int(trl[t, 1])])
        per.append(selected(table, a, max(a, b), channels, units))
    pairs = sorted({(int(c), int(u)) for blk in per for c, u in blk[:, 1:]})
    columns = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    out = [trial_psth(blk, trl[t, 0], trl[t, 1], trl[t, 2], pairs, edges, output, samplerate)
           for t, blk in zip(trial_ids, per)]
    return columns, np.concatenate(out, axis=0)


def ulp_distance(a, b):
    """largest distance in float32 units in the last place between the non-NaN entries of a and b"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ok = ~np.isnan(a)
    if not ok.any():
        return 0
    ia, ib = a[ok].view(np.int32).astype(np.int64), b[ok].view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


def assert_psth(got, ref, output, what=""):
    """spikecount and rate: bit for bit; proportion: within 2 float32 ulp with identical NaN positions"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32, f"{what}: {got.shape} {got.dtype} vs {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN positions"
    if output == "proportion":
        d = ulp_distance(got, ref)
        print(f"{what}: {d} ulp")
        assert d <= 2, f"{what}: {d} ulp"
    else:
        assert np.array_equal(got, ref, equal_nan=True), f"{what}: not bit-identical"
