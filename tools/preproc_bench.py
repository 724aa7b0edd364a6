"""Time the preprocessing kernels on the headline shape (256 channels x 4096 samples x 1000 trials): device-resident
batches through the backend wrappers (event timing, warm-up, median of repeats) and spy.preprocessing from host memory.

    python tools/preproc_bench.py [ntrials]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import syncopy_amd as spy  # noqa: E402
from syncopy_amd import backend  # noqa: E402
from syncopy_amd.preproc import design  # noqa: E402


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


def main(T=1000, N=4096, Cn=256, chunk=125):
    x = torch.randn((chunk, N, Cn), dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    nan = torch.zeros(chunk, dtype=torch.int32, device="cuda")
    sos, zi, edge = design.butterworth(4, [20, 80], "bp", 1000.0)
    work = torch.empty(chunk * (N + 2 * edge) * Cn, dtype=torch.float64, device="cuda")
    taps = torch.from_numpy(design.windowed_sinc("hamming", 1000, np.array([0.045, 0.055]), "bs")).cuda()
    scale = T / chunk
    print(f"device-resident, {chunk} trials per launch, scaled to {T} trials:")
    print(f"  but bp order 4 twopass : {scale * timed(lambda: backend.sosfiltfilt(x, out, sos, zi, edge, nan, work=work)):9.2f} ms")
    print(f"  firws bs order 1000    : {scale * timed(lambda: backend.fir_same(x, out, taps, nan), reps=3):9.2f} ms")
    print(f"  zscore                 : {scale * timed(lambda: backend.standardize(x, out, nan)):9.2f} ms")
    del work
    host = np.random.default_rng(0).normal(size=(chunk * N, Cn)).astype(np.float32)
    e = np.arange(chunk + 1) * N
    data = spy.AnalogData(host, samplerate=1000.0, trialdefinition=np.stack([e[:-1], e[1:], np.zeros(chunk)], 1))
    for name, kw in (("but bp order 4 twopass", dict(filter_type="bp", freq=[20, 80])),
                     ("firws bs order 1000", dict(filter_class="firws", filter_type="bs", freq=[45, 55], order=1000)),
                     ("zscore", dict(filter_class=None, zscore=True))):
        spy.preprocessing(data, **kw).data
        t0 = time.perf_counter()
        spy.preprocessing(data, **kw).data
        print(f"  spy.preprocessing from host memory, {name}: {scale * (time.perf_counter() - t0) * 1e3:9.1f} ms (x{scale:g} of {chunk} trials)")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
