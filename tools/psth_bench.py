"""Time spy.spike_psth on 1000 trials of synthdata.poisson_noise at three sizes: the generator's default (10^4 spikes, 3
channels x 10 units, 'rice' bins), 10^7 spikes with 50 ms bins, and 384 channels x 4 units (10^6 spikes, 'rice' bins).
Per stage - the upload of the table, each kernel on the resident table, the front end as a whole with the table resident
and from host memory - the time (event timing, one warm-up, median of repeats with their spread) and the bytes per
second it stands for when the table is read once at 16 bytes per spike, next to an MI355X's measured HBM copy rate of
6.29 TB/s.

    python tools/psth_bench.py [size ...]          # sizes: default, spikes1e7, chan384
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import syncopy_amd as spy  # noqa: E402
from syncopy_amd import backend  # noqa: E402
from syncopy_amd.statistics import spike_psth as SP  # noqa: E402

HBM_BYTES = 6.29e12
SIZES = {
    "default": (dict(nTrials=1000, seed=1), dict()),
    "spikes1e7": (dict(nTrials=1000, nSpikes=10_000_000, seed=1), dict(binsize=0.05)),
    "chan384": (dict(nTrials=1000, nSpikes=1_000_000, nChannels=384, nUnits=4, seed=1), dict()),
}


def timed(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run(size):
    gen, kw = SIZES[size]
    t0 = time.perf_counter()
    data = spy.synthdata.poisson_noise(**gen)
    nspikes = data.data.shape[0]
    floor = 16.0 * nspikes
    print(json.dumps(dict(size=size, spikes=nspikes, generator_s=time.perf_counter() - t0,
                          read_floor_ms=floor / HBM_BYTES * 1e3)), flush=True)

    def case(name, fn, reps=7):
        med, lo, hi = timed(fn, reps)
        print(json.dumps(dict(size=size, stage=name, ms=med, min=lo, max=hi, table_gbyte_per_s=floor / med * 1e-6)),
              flush=True)

    def upload():
        data.invalidate()
        data.device_columns()
    case("upload of the table (pageable host memory)", upload, reps=3)

    sample, chan, unit = data.device_columns()
    plan = SP._plan(data, kw.get("binsize", "rice"), "proportion", "maxperiod", True, presence=SP._device_presence(data))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(sample.device)      # noqa: E731
    row_lo, row_hi, start, onset = up(plan.row_lo), up(plan.row_hi), up(plan.start), up(plan.onset)
    lohi, lut, edges = up(plan.lohi), up(plan.lut), up(plan.edges)
    chan_ok, unit_ok, unit_k, col_k = up(plan.chan_ok), up(plan.unit_ok), up(plan.unit_k), up(plan.col_k)
    max_rows = int((plan.row_hi - plan.row_lo).max())
    print(json.dumps(dict(size=size, trials=len(plan.trial_ids), bins=plan.nbins, columns=plan.ncols)), flush=True)
    case("psth_presence", lambda: backend.psth_presence(chan, unit, row_lo, row_hi, max_rows, chan_ok, unit_ok))
    case("psth_bin_rows", lambda: backend.psth_bin_rows(sample, row_lo, row_hi, start, onset, edges, plan.samplerate))
    rows = backend.psth_bin_rows(sample, row_lo, row_hi, start, onset, edges, plan.samplerate)
    case("psth_count", lambda: backend.psth_count(chan, unit, rows, lut, plan.C, plan.U, lohi, plan.ncols, 1.0))
    out = backend.psth_count(chan, unit, rows, lut, plan.C, plan.U, lohi, plan.ncols, 1.0)
    case("psth_proportion (unit counts + normalisation)",
         lambda: backend.psth_proportion(chan, unit, row_lo, row_hi, rows, lut, plan.C, plan.U, unit_k, col_k, plan.nk,
                                         edges, out))
    del rows, out
    for output in ("rate", "proportion"):
        case(f"spike_psth(output={output!r}), table resident", lambda: spy.spike_psth(data, output=output, **kw), reps=3)
    case("spike_psth(output='rate', keeptrials=False), table resident",
         lambda: spy.spike_psth(data, keeptrials=False, **kw), reps=3)

    def from_host():
        data.invalidate()
        spy.spike_psth(data, **kw)
    case("spike_psth(output='rate') from host memory", from_host, reps=3)


if __name__ == "__main__":
    backend.require_gpu()
    for name in (sys.argv[1:] or list(SIZES)):
        run(name)
