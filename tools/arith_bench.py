"""Time the operator arithmetic on resident data objects beside torch's own element-wise kernels on the same tensors:
`x + 1.0`, `x * w` (w one weight per channel, broadcast over time) and `x - y` (two objects) on a float32 AnalogData of
256 channels x 4096 samples x 1000 trials, and on a complex64 CrossSpectralData of 1 x 2049 x 256 x 256.

Per case three figures, each the median over rounds of a window of `reps` calls between two device events (one warm-up
round; the three alternate inside a round, so that they see the same machine): the operator as the user writes it (front
end, row table and launch), the kernel alone (backend.arith on a table that is already built), and torch's add / mul /
sub into a fresh tensor.  Bytes are the ones the operation has to move (read the base, read a full operand, write the
result) and the rates are those bytes over the time; an MI355X copies at 6.29 TB/s measured (tools/hbm_rw_probe.hip).
Writes one JSON line per case to profiles/arith_bench.jsonl.

    python tools/arith_bench.py [--trials 1000] [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import syncopy_amd as spy  # noqa: E402
from syncopy_amd import backend  # noqa: E402
from syncopy_amd.datatype import arithmetic as A  # noqa: E402

HBM_BYTES = 6.29e12


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


def kernel_call(plan, base_t, operand_t=None):
    """the launch the front end makes for `plan` from resident tensors, with its table built once"""
    n = np.array([b - a for a, b in plan.rows], dtype=np.int64)
    a0 = np.array([a for a, _ in plan.rows], dtype=np.int64)
    brow = plan.starts if plan.other is None else np.array([a for a, _ in plan.other.rows], dtype=np.int64)
    desc = np.stack([plan.starts, a0, brow, n], axis=1)
    out = torch.empty((plan.nrows,) + plan.inner, dtype=base_t.dtype, device=base_t.device)
    array = None if plan.array is None else torch.from_numpy(plan.array).to(base_t.device)
    return lambda: backend.arith(plan.op, base_t, desc, out, plan.scalar, array, operand_t)


def cases(kind, x, y, xt, yt, w):
    """name -> (operator call, plan, operand tensor of the kernel call, torch call, bytes moved)"""
    wt = torch.from_numpy(w).to(xt.device)
    one = xt.numel() * xt.element_size()
    return {
        f"{kind}: x + 1.0": (lambda: x + 1.0, A._plan(x, 1.0, "+"), None, lambda: torch.add(xt, 1.0), 2 * one),
        f"{kind}: x * w": (lambda: x * w, A._plan(x, w, "*"), None, lambda: torch.mul(xt, wt), 2 * one),
        f"{kind}: x - y": (lambda: x - y, A._plan(x, y, "-"), yt, lambda: torch.sub(xt, yt), 3 * one),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arith_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    lines = []

    def analog():
        nsamp, nchan = 4096, 256
        starts = np.arange(args.trials) * nsamp
        trl = np.stack([starts, starts + nsamp, np.zeros(args.trials)], axis=1)
        objs, tensors = [], []
        for _ in range(2):
            t = torch.randn((args.trials * nsamp, nchan), generator=gen, device=dev, dtype=torch.float32)
            o = spy.AnalogData(None, samplerate=1000.0)
            o.trialdefinition = trl
            o.channel = np.array([f"ch{c}" for c in range(nchan)])
            o.adopt_device_result(t)
            objs.append(o)
            tensors.append(t)
        w = np.linspace(0.5, 1.5, nchan).astype(np.float32)
        return cases(f"AnalogData float32 {nchan} ch x {nsamp} x {args.trials} trials", *objs, *tensors, w)

    def cross():
        shape = (1, 2049, 256, 256)
        objs, tensors = [], []
        for _ in range(2):
            t = torch.view_as_complex(torch.randn(shape + (2,), generator=gen, device=dev, dtype=torch.float32))
            o = spy.CrossSpectralData(None, samplerate=1000.0)
            o.trialdefinition = np.array([[0, 1, 0]])
            o.set_pending(lambda t=t: backend.to_host(t), shape, np.complex64)
            o._dev = t
            objs.append(o)
            tensors.append(t)
        w = (np.linspace(0.5, 1.5, 256) + 0.25j).astype(np.complex64)
        return cases("CrossSpectralData complex64 1 x 2049 x 256 x 256", *objs, *tensors, w)

    for build in (analog, cross):
        for name, (operator, plan, operand_t, torch_call, nbytes) in build().items():
            base_t = A._resident(plan.base)[0]
            res = compare({"operator": operator, "kernel": kernel_call(plan, base_t, operand_t), "torch": torch_call},
                          args.reps, args.rounds)
            line = dict(case=name, bytes=nbytes, floor_ms=nbytes / HBM_BYTES * 1e3, reps=args.reps, rounds=args.rounds)
            for k, (med, lo, hi) in res.items():
                line[k + "_ms"], line[k + "_min_ms"], line[k + "_max_ms"] = med, lo, hi
                line[k + "_tbyte_per_s"] = nbytes / med * 1e-9
            line["kernel_over_torch"] = res["kernel"][0] / res["torch"][0]
            line["operator_over_torch"] = res["operator"][0] / res["torch"][0]
            print(json.dumps(line), flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
