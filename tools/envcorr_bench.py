"""Time the envelope correlations (K12: envcorr_accumulate + envcorr_finalize for amplcorr, powcorr and powcorr_ortho)
beside K7 (ppc_accumulate + ppc_finalize) and K10 (phaselag_accumulate + phaselag_finalize) on the same resident tapered
spectra: 256 channels x 2049 frequencies x 7 tapers, in batches of trials.

Per batch size one figure per call, each the median over rounds of a window of `reps` calls between two device events
(one warm-up round; the calls take turns inside a round, so that they see the same machine): the five accumulations into
zeroed accumulators that exist already, and the five finalizers.  What bounds an accumulation: the spectra, read once per
tile row they belong to (staged_bytes; the floor counts each once), the read-modify-write of the accumulator - float64,
one plane for amplcorr and powcorr, five for powcorr_ortho - and the arithmetic per pair and repetition: one float64 FMA
for amplcorr and powcorr, about 13 vector instructions for powcorr_ortho (5 float32, 3 conversions, 5 float64), against 4
and 2 float32 FMAs in K7 and K10.  An MI355X copies at 6.29 TB/s measured (tools/hbm_rw_probe.hip).
Writes one JSON line per batch size to profiles/envcorr_bench.jsonl.

    python tools/envcorr_bench.py [--batches 4 16 64] [--reps 5] [--rounds 7]
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
MEASURES = ("amplcorr", "powcorr", "powcorr_ortho")


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
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envcorr_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.zeros((F, C, C), dtype=torch.complex64, device=dev)
    acc = torch.zeros((F, C, C, 4), dtype=torch.float32, device=dev)
    # the one-plane accumulator of amplcorr and powcorr is the first plane of powcorr_ortho's five (the calls take turns)
    pair = torch.zeros((5, F, C, C), dtype=torch.float64, device=dev)
    chan = torch.zeros((F, C, 2), dtype=torch.float64, device=dev)
    nt = (C + 31) // 32
    tiles = nt * (nt + 1) // 2
    lines = []
    for T in args.batches:
        spec = torch.view_as_complex(torch.randn((T * K, F, C, 2), generator=gen, device=dev, dtype=torch.float32))
        fns = {"ppc_accumulate": lambda: backend.ppc_accumulate(spec, K, U),
               "phaselag_accumulate": lambda: backend.phaselag_accumulate(spec, K, acc),
               "ppc_finalize": lambda: backend.ppc_finalize(U, 1000, True),
               "phaselag_finalize": lambda: backend.phaselag_finalize(acc, 1000, True, "wpli_debiased")}
        for m in MEASURES:
            p = pair[:backend.ENVCORR_PLANES[m]]
            fns[m + "_accumulate"] = lambda m=m, p=p: backend.envcorr_accumulate(spec, K, p, chan, m)
            fns[m + "_finalize"] = lambda m=m, p=p: backend.envcorr_finalize(p, chan, 7000, m)
        res = compare(fns, args.reps, args.rounds)
        spec_bytes = spec.numel() * 8
        pairs = T * K * F * tiles * 1024
        line = dict(case=f"{C} channels x {F} frequencies x {K} tapers x {T} trials", trials=T, reps=args.reps, rounds=args.rounds,
                    spectra_bytes=spec_bytes, spectra_floor_ms=spec_bytes / HBM_BYTES * 1e3,
                    staged_bytes=T * K * F * tiles * 64 * 8,                                   # what the tiles pull from memory
                    ppc_accumulator_bytes=2 * U.numel() * 8, phaselag_accumulator_bytes=2 * acc.numel() * 4,
                    envcorr_accumulator_bytes=2 * F * tiles * 1024 * 8, envcorr_ortho_accumulator_bytes=2 * 5 * F * tiles * 1024 * 8,
                    pair_repetitions=pairs)
        for name, (med, lo, hi) in res.items():
            line[name + "_ms"], line[name + "_min_ms"], line[name + "_max_ms"] = med, lo, hi
        for m in MEASURES:
            line[m + "_ms_per_trial"] = res[m + "_accumulate"][0] / T
            line[m + "_over_ppc"] = res[m + "_accumulate"][0] / res["ppc_accumulate"][0]
            line[m + "_over_phaselag"] = res[m + "_accumulate"][0] / res["phaselag_accumulate"][0]
            line[m + "_finalize_over_ppc"] = res[m + "_finalize"][0] / res["ppc_finalize"][0]
            line[m + "_pair_repetitions_per_ns"] = pairs / (res[m + "_accumulate"][0] * 1e6)
        line["ppc_ms_per_trial"] = res["ppc_accumulate"][0] / T
        line["phaselag_ms_per_trial"] = res["phaselag_accumulate"][0] / T
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
