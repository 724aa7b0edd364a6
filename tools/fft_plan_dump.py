"""Kernel name and a hash of the output bytes of the tapered-FFT plan over a fixed seeded matrix of transform lengths: two
builds of the library that choose and launch the same kernels write the same file, byte for byte.

    PYTHONPATH=. python tools/fft_plan_dump.py OUT.json [--lib PATH/libspyhip.so]
"""
import hashlib
import json
import sys

import numpy as np
import torch

from syncopy_amd import _lib

if "--lib" in sys.argv:
    _lib.LIB_PATH = sys.argv[sys.argv.index("--lib") + 1]
from syncopy_amd import backend as be

# one length per kernel family and edge of the route, then every scheduled length (float32, HALF, float64)
ROUTE = [256, 4096, 8192, 16384, 128, 360, 2000, 5000, 10000, 1009, 4093, 4097, 4116, 11000, 12000, 20480, 24000, 32768, 65536]
DEC = [100, 200, 300, 400, 500, 600, 768, 800, 1000, 1200, 1500, 1536, 1600, 2000, 2400, 2500, 3000, 3072, 3200, 4000,
       4800, 5000, 6000, 6144, 7500, 8000, 10000]
HALF = [12000, 12288, 15000, 16000, 16384, 20000]
DEC64 = [256, 512, 1024, 2048, 4096, 8192] + DEC
LENGTHS = list(dict.fromkeys(ROUTE + DEC + HALF + DEC64))
GAP = 37


def run(res, tag, nfft, nchan, output, keep, extras=False):
    rng = np.random.default_rng(nfft)
    data = torch.from_numpy(rng.normal(size=(2 * nfft + GAP + 5, nchan)).astype(np.float32) + 0.25).cuda()
    starts = torch.tensor([3, 3 + nfft + GAP], dtype=torch.int64, device="cuda")
    n = np.arange(nfft)
    hann = np.hanning(nfft)
    tapers = np.stack([hann, hann * np.sin(2 * np.pi * 3 * n / nfft)])
    plan = be.FFTPlan(nfft, nfft, nchan, tapers, np.sqrt(2.0) / nfft, 0 if extras else None, False, None, output, keep,
                      reference_mean=extras)
    for prec in ("f32", "f64"):
        if prec == "f64" and not plan.set_precision(True):
            continue
        absmax = torch.zeros(nchan, dtype=torch.float32, device="cuda") if extras else None
        out = plan.execute(data, starts, absmax=absmax)
        torch.cuda.synchronize()
        h = hashlib.sha256(out.cpu().numpy().tobytes())
        if extras:
            h.update(absmax.cpu().numpy().tobytes())
        res[f"{tag}_{prec}"] = [plan.kernel_name, h.hexdigest()]


def main():
    be.require_gpu()
    res = {}
    for i, nfft in enumerate(LENGTHS):
        output, keep = (("pow", False), ("fourier", True))[i % 2]
        run(res, f"N{nfft}_{output}_{'keep' if keep else 'mean'}", nfft, 5, output, keep)
    run(res, "N2000_C8_fourier_keep", 2000, 8, "fourier", True)
    for nfft in (4096, 12000):
        run(res, f"N{nfft}_absmax_refmean", nfft, 5, "fourier", True, extras=True)
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(len(res), "cases ->", sys.argv[1])


if __name__ == "__main__":
    main()
