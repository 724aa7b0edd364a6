"""Time the phase slope index (K13: spyhip_phaseslope_from_accumulator) beside K5 (spyhip_coh_from_accumulator, output
'imag') on the same resident raw accumulator: 256 channels x 2049 frequencies, half widths 1, 8, 64 and 0 (the whole axis).

One figure per call, each the median over rounds of a window of `reps` calls between two device events (one warm-up
round; the calls take turns inside a round, so that they see the same machine), into outputs that exist already.  What
bounds either kernel from below: 8 bytes read and 2 x 4 bytes written per element of the lower triangle at tile
granularity (floor_bytes; K13 with h = 0 writes one plane only).  K13 reads every bin a second time 2h bins later (from the
L2 or the Infinity Cache where the run's window still sits there) and the halo of 2h bins of every frequency run.  An
MI355X copies at 6.29 TB/s measured (tools/hbm_rw_probe.hip).  Writes one JSON line to profiles/phaseslope_bench.jsonl.

    python tools/phaseslope_bench.py [--halves 1 8 64 0] [--reps 5] [--rounds 7]
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
C, F, ROWS = 256, 2049, 28


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
    ap.add_argument("--halves", type=int, nargs="+", default=[1, 8, 64, 0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phaseslope_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    spec = torch.view_as_complex(torch.randn((ROWS, F, C, 2), generator=gen, device=dev, dtype=torch.float32))
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device=dev)
    backend.csd_accumulate(spec, acc)
    del spec
    scale = 1.0 / ROWS
    coh = torch.empty((F, C, C), dtype=torch.float32, device=dev)
    psi = torch.empty((F, C, C), dtype=torch.float32, device=dev)
    fns = {"coh_imag": lambda: backend.coh_from_accumulator(acc, scale, "imag", out=coh)}
    for h in args.halves:
        fns[f"psi_h{h}"] = lambda h=h: backend.phase_slope_from_accumulator(acc, scale, h, out=psi if h else psi[:1])
    res = compare(fns, args.reps, args.rounds)
    nt = (C + 31) // 32
    elements = F * (nt * (nt + 1) // 2) * 1024
    floor = elements * 16
    line = dict(case=f"{C} channels x {F} frequencies, raw accumulator of {ROWS} rows", reps=args.reps, rounds=args.rounds,
                lower_triangle_elements=elements, floor_bytes=floor, floor_ms=floor / HBM_BYTES * 1e3)
    for name, (med, lo, hi) in res.items():
        line[name + "_ms"], line[name + "_min_ms"], line[name + "_max_ms"] = med, lo, hi
        nbytes = elements * 8 + (C * C * 4 if name == "psi_h0" else elements * 8)
        line[name + "_floor_bytes_per_s"] = nbytes / (med * 1e-3)
        if name != "coh_imag":
            line[name + "_over_coh_imag"] = med / res["coh_imag"][0]
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
