"""Record tests/golden/psth.npz: results of the reference's own single-trial histogram (statistics/psth.py: psth), loaded
by file path (it needs only NumPy and SciPy).

    python tools/record_psth_golden.py <path to the reference's syncopy/statistics directory>

Every case is one trial that holds spikes on all its channels 0 .. C-1: there the reference's channel bins and the
columns (channel, unit) agree (see the deviation in syncopy_amd/statistics/spike_psth.py).  Stored per case: the spikes
(n, 3) [sample, channel, unit], par = [start, end, onset, samplerate], the float64 edges, the columns, and
psth(...)[0].astype(float32) for the three outputs.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("rate", "spikecount", "proportion")


def _load(folder):
    spec = importlib.util.spec_from_file_location("reference_psth", os.path.join(folder, "psth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spikes(rng, n, start, end, nchan, nunit, dup=False):
    """n spikes inside [start, end), every channel present, sorted by sample"""
    samples = rng.integers(start, end, size=n)
    if dup:
        samples = start + (samples - start) // 97 * 97          # many equal sample numbers
    chan = rng.integers(0, nchan, size=n)
    chan[:nchan] = np.arange(nchan)
    unit = rng.integers(0, nunit, size=n)
    tab = np.stack([samples, chan, unit], axis=1).astype(np.int64)
    return tab[np.argsort(tab[:, 0], kind="stable")]


def _combs(tab, extra=()):
    pairs = {(int(c), int(u)) for c, u in tab[:, 1:]} | set(extra)
    return np.array(sorted(pairs), dtype=np.int64)


def cases():
    rng = np.random.default_rng(20261018)
    out = {}

    def add(name, tab, start, end, onset, fs, edges, extra=()):
        out[name] = (tab, np.array([start, end, onset, fs], dtype=np.float64), np.asarray(edges, dtype=np.float64),
                     _combs(tab, extra))

    # both edge styles at the three samplerates; the window is the trial's own [first, last] sample time
    for tag, fs, start, n, onset in (("1k", 1000.0, 100, 1000, -200), ("30k", 30000.0, 3_000_000, 30000, -6000),
                                     ("24k", 24414.0625, 50_000, 24414, -4883)):
        tab = _spikes(rng, 300, start, start + n, 3, 4)
        w0, w1 = onset / fs, (n - 1 + onset) / fs
        add(f"lin_{tag}", tab, start, start + n, onset, fs, np.linspace(w0, w1, 13))
        bs = 0.05 if tag == "1k" else 0.0137
        add(f"arange_{tag}", tab, start, start + n, onset, fs, np.arange(w0, w1 + bs, bs))
    # a window that starts before and ends after the trial: NaN head and tail
    tab = _spikes(rng, 200, 100, 1100, 2, 3)
    add("nan_head_tail", tab, 100, 1100, -200, 1000.0, np.arange(-0.5, 1.2 + 0.1, 0.1))
    # ... wholly behind / wholly before the trial: all NaN
    add("window_behind", tab, 100, 1100, -200, 1000.0, np.arange(2.0, 3.0 + 0.25, 0.25))
    add("window_before", tab, 100, 1100, -200, 1000.0, np.linspace(-3.0, -2.0, 5))
    # a spike exactly on the last edge (t = 0.5 = edges[-1]), the trial going on behind it
    tab = _spikes(rng, 120, 0, 500, 2, 2)
    tab = np.concatenate([tab, [[500, 1, 0], [500, 0, 1], [501, 0, 0], [650, 1, 1]]]).astype(np.int64)
    add("last_edge", tab, 0, 800, 0, 1000.0, np.linspace(0.0, 0.5, 6))
    # columns absent from the trial: a unit that never occurs, and a unit that occurs on another channel only
    tab = _spikes(rng, 150, 0, 1000, 3, 3)
    tab = tab[~((tab[:, 1] == 2) & (tab[:, 2] == 1))]
    add("absent_column", tab, 0, 1000, -100, 1000.0, np.arange(-0.1, 0.899 + 0.1, 0.1), extra=[(1, 7), (2, 1)])
    # a unit whose spikes all lie outside the window: NaN column under "proportion"
    tab = _spikes(rng, 150, 0, 1000, 2, 3)
    tab = tab[(tab[:, 2] != 2) | (tab[:, 0] >= 400)]
    add("unit_outside_window", tab, 0, 1000, 0, 1000.0, np.linspace(0.0, 0.3, 7))
    # many equal sample numbers, at a rate that is no integer
    tab = _spikes(rng, 400, 7000, 19000, 3, 2, dup=True)
    add("equal_samples", tab, 7000, 19000, -2000, 24414.0625, np.arange(-0.05, 0.4 + 0.03, 0.03))
    # one bin
    tab = _spikes(rng, 40, 0, 300, 2, 2)
    add("one_bin", tab, 0, 300, -50, 1000.0, np.array([-0.05, 0.249]))
    return out


def main(folder):
    ref = _load(folder)
    out = {}
    names = []
    for name, (tab, par, edges, combs) in cases().items():
        assert set(tab[:, 1]) == set(range(int(tab[:, 1].max()) + 1)), name
        names.append(name)
        out[f"{name}_spikes"], out[f"{name}_par"], out[f"{name}_edges"], out[f"{name}_columns"] = tab, par, edges, combs
        for output in OUTPUTS:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                      # 0 / 0 of an empty density histogram
                counts, _ = ref.psth(tab, par[0], par[2], par[1], chan_unit_combs=combs, tbins=edges, output=output,
                                     samplerate=par[3])
            out[f"{name}_{output}"] = counts.astype(np.float32)
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "psth.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
