"""Time the phase-lag accumulation (K10: phaselag_accumulate + phaselag_finalize) beside K7 (ppc_accumulate + ppc_finalize)
on the same resident tapered spectra: 256 channels x 2049 frequencies x 7 tapers, in batches of trials.

Per batch size four figures, each the median over rounds of a window of `reps` calls between two device events (one
warm-up round; the calls alternate inside a round, so that they see the same machine): the two accumulations into zeroed
accumulators that exist already, and the two finalizers.  Bytes are the ones an accumulation has to move - every spectrum
of the batch read once per tile row it belongs to is what the kernels do; the floor counts each once - and the arithmetic
is the FMAs of the taper sums: 4 per pair and taper in K7 (two packed), 2 in K10, over the 32 x 32 tiles of the lower
triangle.  An MI355X copies at 6.29 TB/s measured (tools/hbm_rw_probe.hip).
Writes one JSON line per batch size to profiles/phaselag_bench.jsonl.

    python tools/phaselag_bench.py [--batches 4 16] [--reps 5] [--rounds 7]
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

HBM_BYTES = 6.29e12
C, F, K = 256, 2049, 7


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
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phaselag_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.zeros((F, C, C), dtype=torch.complex64, device=dev)
    acc = torch.zeros((F, C, C, 4), dtype=torch.float32, device=dev)
    nt = (C + 31) // 32
    tiles = nt * (nt + 1) // 2
    lines = []
    for T in args.batches:
        spec = torch.view_as_complex(torch.randn((T * K, F, C, 2), generator=gen, device=dev, dtype=torch.float32))
        fns = {"ppc_accumulate": lambda: backend.ppc_accumulate(spec, K, U),
               "phaselag_accumulate": lambda: backend.phaselag_accumulate(spec, K, acc),
               "ppc_finalize": lambda: backend.ppc_finalize(U, 1000, True),
               "phaselag_finalize": lambda: backend.phaselag_finalize(acc, 1000, True, "wpli_debiased")}
        res = compare(fns, args.reps, args.rounds)
        spec_bytes = spec.numel() * 8
        line = dict(case=f"{C} channels x {F} frequencies x {K} tapers x {T} trials", trials=T, reps=args.reps, rounds=args.rounds,
                    spectra_bytes=spec_bytes, spectra_floor_ms=spec_bytes / HBM_BYTES * 1e3,
                    staged_bytes=T * K * F * tiles * 64 * 8,                                   # what the tiles pull through LDS
                    ppc_accumulator_bytes=2 * U.numel() * 8, phaselag_accumulator_bytes=2 * acc.numel() * 4,
                    ppc_fma=4 * T * K * F * tiles * 1024, phaselag_fma=2 * T * K * F * tiles * 1024)
        for name, (med, lo, hi) in res.items():
            line[name + "_ms"], line[name + "_min_ms"], line[name + "_max_ms"] = med, lo, hi
        line["accumulate_over_ppc"] = res["phaselag_accumulate"][0] / res["ppc_accumulate"][0]
        line["finalize_over_ppc"] = res["phaselag_finalize"][0] / res["ppc_finalize"][0]
        line["ms_per_trial"] = res["phaselag_accumulate"][0] / T
        line["ppc_ms_per_trial"] = res["ppc_accumulate"][0] / T
        print(json.dumps(line), flush=True)
        lines.append(line)
        del spec
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
