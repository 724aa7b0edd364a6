"""A hash of the accumulator bytes of the cross-spectral update over a fixed seeded matrix of shapes and entry points: two
builds of the library that launch the same kernels over the same ranges in the same order write the same file, byte for
byte (the accumulation is deterministic: fixed-order reductions, no atomics).

    PYTHONPATH=. python tools/csd_route_dump.py OUT.json
"""
import hashlib
import json
import sys

import numpy as np
import torch

from syncopy_amd import backend as be

# the shapes of tests/test_gpu_kernels.py::test_csd_accumulate_vs_oracle: every kernel family and its tail
SHAPES = [(5, 33, 14), (16, 101, 140), (40, 17, 35), (70, 9, 64), (256, 5, 70), (256, 259, 10), (128, 131, 20), (64, 1027, 9),
          (192, 300, 12), (160, 259, 10), (224, 6, 13), (96, 515, 9), (32, 2051, 5), (320, 131, 9), (384, 87, 10), (48, 1283, 9),
          (240, 258, 10), (16, 300, 12), (80, 200, 9), (112, 77, 10), (144, 130, 9), (176, 50, 12), (208, 33, 9), (272, 40, 9),
          (288, 9, 20), (304, 17, 9), (336, 12, 9), (352, 9, 9), (368, 8, 10), (400, 9, 9), (416, 7, 9), (432, 10, 9), (448, 10, 9),
          (464, 5, 12), (480, 9, 12), (496, 6, 9), (384, 7, 40), (512, 65, 20), (300, 130, 10), (255, 270, 9), (63, 33, 14),
          (127, 3, 40), (301, 5, 12), (640, 5, 9), (768, 3, 10), (1024, 2, 9), (700, 4, 9), (513, 3, 9), (1025, 2, 5), (528, 70, 8),
          # row-split tails
          (256, 259, 300), (256, 2049, 70)]


def spectra(C, F, R):
    g = torch.Generator().manual_seed(1000 * C + F + R)
    return torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, dtype=torch.float32)).cuda()


def blocked_layout(spec):
    R, F, C = spec.shape
    nq = (C + 3) // 4
    pad = torch.zeros((R, F, 4 * nq), dtype=spec.dtype, device=spec.device)
    pad[:, :, :C] = spec
    return pad.reshape(R, F, nq, 4).permute(0, 2, 1, 3).contiguous()


def record(res, tag, acc):
    torch.cuda.synchronize()
    res[tag] = [hashlib.sha256(acc.cpu().numpy().tobytes()).hexdigest(), be.csd_split_fallbacks()]


def run(res, C, F, R):
    spec = spectra(C, F, R)
    new = lambda: torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    tag = f"C{C}_F{F}_R{R}"
    half = R // 2
    acc = new()
    be.csd_accumulate(spec[:half].contiguous(), acc)          # two launches: accumulation across calls
    be.csd_accumulate(spec[half:].contiguous(), acc)
    record(res, tag, acc)
    record(res, tag + "_f32", be.csd_accumulate(spec, new(), split=False))
    if C == 256:
        absmax = torch.view_as_real(spec).abs().amax(dim=(0, 1, 3)).contiguous()
        record(res, tag + "_absmax", be.csd_accumulate(spec, new(), absmax=absmax))
    try:
        record(res, tag + "_blocked", be.csd_accumulate(blocked_layout(spec), new(), blocked=True))
    except be.SpyHipError as exc:          # (rows too wide for the staging buffer of the blocked layout)
        res[tag + "_blocked"] = [str(exc), 0]
    with be.csd_phase_exact(True):
        record(res, tag + "_exact", be.csd_accumulate(spec, new()))
        record(res, tag + "_exact_f32", be.csd_accumulate(spec, new(), split=False))


def main():
    be.require_gpu()
    res = {}
    for C, F, R in SHAPES:
        run(res, C, F, R)
    # the half-precision update range by range (coh_pipeline), its float32 tail with the last range
    C, F, R = 256, 515, 1024
    spec = spectra(C, F, R)
    absmax = torch.view_as_real(spec).abs().amax(dim=(0, 1, 3)).contiguous()
    ranges = be.frequency_ranges(F)
    acc = be.csd_accumulate(spec, torch.zeros((F, C, C), dtype=torch.complex64, device="cuda"), absmax=absmax, ranges=ranges)
    record(res, f"C{C}_F{F}_R{R}_ranges{len(ranges) if ranges else 0}_events{len(acc.spyhip_range_events or [])}", acc)
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(len(res), "cases ->", sys.argv[1])


if __name__ == "__main__":
    main()
