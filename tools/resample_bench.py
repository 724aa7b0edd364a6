"""Time the resampling kernel on the headline shape (256 channels x 4096 samples x 1000 trials): device-resident batches
through the backend wrappers (event timing, warm-up, median of repeats), with the fused multiply-adds and bytes each case
needs and its lower bound on an MI355X (78.6 TFLOP/s FP64 vector, 6.29 TB/s measured HBM copy rate).

    python tools/resample_bench.py [ntrials]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syncopy_amd import backend  # noqa: E402
from syncopy_amd.preproc import design  # noqa: E402

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


def fmas_per_series(nout, ntaps, up, down):
    """taps an output meets: those of its phase, (m * down + half) % up + j * up < ntaps"""
    half = (ntaps - 1) // 2
    phase = (np.arange(nout) * down + half) % up
    return int(np.sum((ntaps - phase + up - 1) // up * (phase < ntaps)))


def main(T=1000, N=4096, Cn=256, chunk=125):
    x = torch.randn((chunk, N, Cn), dtype=torch.float32, device="cuda")
    tmp = torch.empty_like(x)
    nan = torch.zeros(chunk, dtype=torch.int32, device="cuda")
    scale = T / chunk
    cases = []

    def case(name, taps, up, down, first_pass=False):
        nout = -(-N * up // down)
        out = torch.empty((chunk, nout, Cn), dtype=torch.float32, device="cuda")
        td = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float64)).cuda()

        def run():
            src = backend.fir_same(x, tmp, td, nan) if first_pass else x
            backend.upfirdn(src, out, td, up, down)
        med, lo, hi = timed(run)
        fma = fmas_per_series(nout, len(taps), up, down) + (N * len(taps) if first_pass else 0)
        byts = 4 * (N + nout) + (8 * N if first_pass else 0)
        t_flop = 2.0 * fma * T * Cn / FP64_FLOPS * 1e3
        t_byte = byts * T * Cn / HBM_BYTES * 1e3
        bound = max(t_flop, t_byte)
        row = dict(case=name, ms_per_1000_trials=scale * med, min=scale * lo, max=scale * hi, gflop=2e-9 * fma * T * Cn,
                   gbyte=1e-9 * byts * T * Cn, bound_ms=bound, bound_by="fp64" if t_flop > t_byte else "hbm",
                   fraction_of_bound=bound / (scale * med))
        cases.append(row)
        print(json.dumps(row), flush=True)

    case("resample 1000 -> 600, order 1000", design.windowed_sinc("hamming", 1000, 0.1) * 3, 3, 5)
    case("upfirdn pass alone, 30000 -> 1000, order 1000", design.windowed_sinc("hamming", 1000, 500 / 30000), 1, 30)
    case("downsample 30000 -> 1000, lpfreq 500, order 1000 (fir_same + upfirdn)",
         design.windowed_sinc("hamming", 1000, 500 / 30000), 1, 30, first_pass=True)
    case("downsample by 4", np.ones(1), 1, 4)
    return cases


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
