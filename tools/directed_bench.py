"""Time the directed-measure kernels at the production shape, 2049 frequencies x 256 x 256 complex128: spyhip_zinv (out of
place and in place) and both axes of spyhip_directed_norm (K11), beside what the library already does on the same kind
of array: one spyhip_wilson_g call - the inverse of the Wilson iteration with the two matrix-core products behind it -
and the figures on record for the inverse alone and for granger_kernel, the existing finalizer over the same H
(profiles/r6_wilson_kernel_stats.csv: zinv64_mfma_kernel 7.50 ms per call, granger_kernel 3.94 ms).

Every figure is the median over rounds of a window of `reps` calls between two device events (one warm-up round; the
calls alternate inside a round, so that they see the same machine).  The norm kernel has to read the 16-byte entries once
(2.15 GB) and write the float32 values once (0.54 GB): its achieved bytes per second are these 2.69 GB over its time,
against the 6.29 TB/s an MI355X copies at (tools/hbm_rw_probe.hip).  The matrices are I + 0.3 G / sqrt(n) with complex
Gaussian G (condition numbers below 100; the block kernel's flag stays down), the same for every call.
Writes JSON lines to profiles/directed_bench.jsonl.

    python tools/directed_bench.py [--nfreq 2049] [--n 256] [--reps 5] [--rounds 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from syncopy_amd import backend  # noqa: E402
from syncopy_amd.connectivity.wilson_sharded import HipPrims  # noqa: E402

HBM_BYTES = 6.29e12
ON_RECORD = {"zinv64_mfma_kernel_ms": 7.495, "granger_kernel_ms": 3.936, "source": "profiles/r6_wilson_kernel_stats.csv"}


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(fns, reps, rounds):
    """{name: (median, min, max) ms per call}; the functions take turns inside every round"""
    for fn in fns.values():
        window(fn, 2)
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(window(fn, reps))
    return {name: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfreq", type=int, default=2049)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "directed_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    F, n = args.nfreq, args.n
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    M = torch.view_as_complex(torch.randn((F, n, n, 2), generator=gen, device=dev, dtype=torch.float64)) * (0.3 / np.sqrt(n))
    M += torch.eye(n, dtype=torch.complex128, device=dev)
    M = M.contiguous()
    U = torch.tril(M).contiguous()
    w = torch.rand((n,), generator=gen, device=dev, dtype=torch.float64) + 0.5
    out = torch.empty_like(M)
    work = M.clone()
    prims = HipPrims(dev)

    def in_place():
        work.copy_(M)                      # (timed with it, and on its own below)
        backend.zinv(work, out=work)

    fns = {"zinv": lambda: backend.zinv(M, out=out),
           "zinv_in_place_with_refill": in_place,
           "refill": lambda: work.copy_(M),
           "wilson_g": lambda: prims.g(M, U, False),
           "directed_norm_axis0": lambda: backend.directed_norm(M, None, 0),
           "directed_norm_axis1": lambda: backend.directed_norm(M, None, 1),
           "directed_norm_axis0_weighted_squared": lambda: backend.directed_norm(M, w, 0, True),
           "directed_norm_axis1_weighted_squared": lambda: backend.directed_norm(M, w, 1, True)}
    res = compare(fns, args.reps, args.rounds)
    norm_bytes = F * n * n * (16 + 4)
    line = dict(case=f"{F} frequencies x {n} x {n} complex128", reps=args.reps, rounds=args.rounds, norm_bytes=norm_bytes,
                norm_floor_ms=norm_bytes / HBM_BYTES * 1e3, on_record=ON_RECORD)
    for name, (med, lo, hi) in res.items():
        line[name + "_ms"], line[name + "_min_ms"], line[name + "_max_ms"] = med, lo, hi
    line["zinv_in_place_ms"] = res["zinv_in_place_with_refill"][0] - res["refill"][0]
    for axis in (0, 1):
        line[f"directed_norm_axis{axis}_bytes_per_s"] = norm_bytes / (res[f"directed_norm_axis{axis}"][0] * 1e-3)
        line[f"directed_norm_axis{axis}_of_hbm"] = line[f"directed_norm_axis{axis}_bytes_per_s"] / HBM_BYTES
    if (F, n) == (2049, 256):
        line["zinv_over_inverse_on_record"] = res["zinv"][0] / ON_RECORD["zinv64_mfma_kernel_ms"]
        line["directed_norm_axis0_over_granger_kernel_on_record"] = res["directed_norm_axis0"][0] / ON_RECORD["granger_kernel_ms"]
        line["directed_norm_axis1_over_granger_kernel_on_record"] = res["directed_norm_axis1"][0] / ON_RECORD["granger_kernel_ms"]
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
