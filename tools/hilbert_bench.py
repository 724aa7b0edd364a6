"""Time the Hilbert kernels of spy.preprocessing (csrc/hilbert.hip): device-resident batches through backend.hilbert
(event timing, warm-up, median of repeats), 125 trials of 256 channels per launch scaled to 1000 trials, at 4096 samples
(PACKED), 1000 (BLUE) and 10000 (ANY64), next to the byte bound of the kernel's traffic and to SciPy on one host core.

    python tools/hilbert_bench.py [--json FILE]
"""
import json
import os
import sys
import time

import numpy as np
import scipy.signal as sps
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syncopy_amd import backend  # noqa: E402

HBM_BYTES_PER_S = 3.6e12        # what a streaming kernel reaches on an MI355X


def timed(fn, reps=5):
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
    return float(np.median(ms))


def scipy_ms_per_trial(N, Cn):
    x = np.random.default_rng(0).normal(size=(N, Cn)).astype(np.float32)
    sps.hilbert(x, axis=0)
    t0 = time.perf_counter()
    np.abs(sps.hilbert(x, axis=0))
    return (time.perf_counter() - t0) * 1e3


def main(T=1000, Cn=256, chunk=125):
    rows = []
    for N, reps in ((4096, 5), (1000, 5), (10000, 3)):
        x = torch.randn((chunk, N, Cn), dtype=torch.float32, device="cuda")
        nan = torch.zeros(chunk, dtype=torch.int32, device="cuda")
        name = backend.hilbert_plan(N, x.device).kernel_name
        for output in ("abs", "complex"):
            out = torch.empty(x.shape, dtype=torch.complex64 if output == "complex" else torch.float32, device="cuda")
            ms = T / chunk * timed(lambda: backend.hilbert(x, out, output, nan), reps)
            nbytes = T * N * Cn * (4 + (8 if output == "complex" else 4))
            rows.append(dict(nsamp=N, output=output, kernel=name, ms_per_1000_trials=ms,
                             byte_bound_ms=nbytes / HBM_BYTES_PER_S * 1e3))
            del out
        rows[-1]["scipy_one_core_ms_per_1000_trials"] = rows[-2]["scipy_one_core_ms_per_1000_trials"] = \
            T * scipy_ms_per_trial(N, Cn)
        del x
    for r in rows:
        print(f"N={r['nsamp']:6d} {r['output']:8s} {r['ms_per_1000_trials']:10.2f} ms per {T} trials x {Cn} channels "
              f"(byte bound {r['byte_bound_ms']:.2f} ms, SciPy abs on one core {r['scipy_one_core_ms_per_1000_trials']:.0f} ms)"
              f"  {r['kernel']}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
