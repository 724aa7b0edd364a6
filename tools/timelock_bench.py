"""Time spy.timelockanalysis on the headline shape (256 channels x 4096 samples x 1000 trials, float32): the covariance
kernel alone on a resident batch, timelockanalysis(covariance=True) from data resident on the device, and the same from
pageable host memory (event timing, one warm-up, median of repeats with their spread), next to the lower bounds on an
MI355X (78.6 TFLOP/s FP64 matrix, 6.29 TB/s measured HBM copy rate).  125 trials are resident; the times are scaled by 8.

    python tools/timelock_bench.py [ntrials]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import syncopy_amd as spy  # noqa: E402
from syncopy_amd import backend  # noqa: E402

FP64_FLOPS = 78.6e12
HBM_BYTES = 6.29e12


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


def main(T=1000, N=4096, Cn=256, chunk=125):
    backend.require_gpu()
    scale = T / chunk
    rng = np.random.default_rng(0)
    host = rng.standard_normal((chunk * N, Cn), dtype=np.float32)
    e = np.arange(chunk + 1) * N
    trl = np.stack([e[:-1], e[1:], np.zeros(chunk)], axis=1)
    tiles = (Cn + 15) // 16
    # the 16 x 16 tiles on or below the diagonal, a multiply-add per sample and element; the trials read once by the
    # mean and once by the products, the matrices written once
    flop = 2.0 * (tiles * (tiles + 1) // 2) * 256 * N * T
    byts = (2 * 4 * N * Cn + 4 * Cn * Cn) * T
    bounds = dict(gflop=1e-9 * flop, gbyte=1e-9 * byts, fp64_bound_ms=flop / FP64_FLOPS * 1e3,
                  hbm_bound_ms=byts / HBM_BYTES * 1e3)
    rows = []

    def case(name, fn, reps=7, **more):
        med, lo, hi = timed(fn, reps)
        row = dict(case=name, ms_per_1000_trials=scale * med, min=scale * lo, max=scale * hi, **more)
        rows.append(row)
        print(json.dumps(row), flush=True)

    x = torch.from_numpy(host).cuda().view(chunk, N, Cn)
    out = torch.empty((chunk, Cn, Cn), dtype=torch.float32, device="cuda")
    case("covariance kernel alone (column means + products)", lambda: backend.cov(x, None, out=out), **bounds)
    del x, out

    resident = spy.AnalogData(host, samplerate=1000.0, trialdefinition=trl)
    resident.device_data()
    torch.cuda.synchronize()
    case("timelockanalysis(covariance=True), data resident on the device",
         lambda: spy.timelockanalysis(resident, covariance=True))
    case("timelockanalysis(covariance=False), data resident on the device", lambda: spy.timelockanalysis(resident))
    del resident

    def from_host():
        spy.timelockanalysis(spy.AnalogData(host, samplerate=1000.0, trialdefinition=trl), covariance=True)
    case("timelockanalysis(covariance=True) from pageable host memory", from_host, reps=3)
    return rows


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
