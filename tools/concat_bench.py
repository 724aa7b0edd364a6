"""Time spy.concat on resident data objects beside torch.cat on the same tensors.

  (A) 2 x float32 AnalogData of 128 channels x 4096 samples x 1000 trials -> 256 channels: runs of 512 bytes;
  (B) 4 x 64 channels of the same recording length -> 256 channels: runs of 256 bytes;
  (C) 2 x complex64 SpectralData of (1000, 7, 2049, 32), the default dimord -> 64 channels: 7 x 2049 lines per row.

Per case three figures, each the median over rounds of a window of `reps` calls between two device events (one warm-up
round; the three alternate inside a round, so that they see the same machine): the front end as the user writes it
(planner, row table and launch), the kernel alone (backend.concat on a table that is already built), and
`torch.cat(..., dim=-1)` into a fresh tensor.  Bytes are the ones the operation has to move (read every source, write the
result) and the rates are those bytes over the time; an MI355X copies at 6.29 TB/s measured (tools/hbm_rw_probe.hip).
Writes one JSON line per case to profiles/concat_bench.jsonl.

    python tools/concat_bench.py [--trials 1000] [--reps 10] [--rounds 7]
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
from syncopy_amd.datatype import concat as K  # noqa: E402
from syncopy_amd.datatype.arithmetic import _resident  # noqa: E402

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


def kernel_call(plan, sources):
    """the launch the front end makes for `plan` from the resident tensors, with its table built once"""
    desc = np.stack([plan.starts, plan.n] + [np.array([a for a, _ in rows], dtype=np.int64) for rows in plan.rows], axis=1)
    out = torch.empty((plan.nrows,) + plan.inner, dtype=sources[0].dtype, device=sources[0].device)
    return lambda: backend.concat(sources, desc, out, plan.pre), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concat_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    T = args.trials
    lines = []

    def analog(nobj, nchan):
        nsamp = 4096
        starts = np.arange(T) * nsamp
        objs, tensors = [], []
        for k in range(nobj):
            t = torch.randn((T * nsamp, nchan), generator=gen, device=dev, dtype=torch.float32)
            x = spy.AnalogData(None, samplerate=1000.0)
            x.trialdefinition = np.stack([starts, starts + nsamp, np.full(T, -nsamp // 2)], axis=1)
            x.channel = np.array([f"probe{k}_{c}" for c in range(nchan)])
            x.adopt_device_result(t)
            objs.append(x)
            tensors.append(t)
        return f"{nobj} x AnalogData float32 {nchan} ch x {nsamp} x {T} trials -> {nobj * nchan} ch", objs, tensors

    def spectral():
        shape = (T, 7, 2049, 32)
        objs, tensors = [], []
        for k in range(2):
            t = torch.view_as_complex(torch.randn(shape + (2,), generator=gen, device=dev, dtype=torch.float32))
            s = spy.SpectralData(None, samplerate=2048.0)
            s.trialdefinition = np.stack([np.arange(T), np.arange(T) + 1, np.zeros(T)], axis=1)
            s.freq, s.taper = np.arange(2049) * 0.5, np.array([f"taper{i}" for i in range(7)])
            s.channel = np.array([f"probe{k}_{c}" for c in range(32)])
            s.set_pending(lambda t=t: backend.to_host(t), shape, np.complex64)
            s._resident = t
            objs.append(s)
            tensors.append(t)
        return f"2 x SpectralData complex64 {T} x 7 x 2049 x 32 -> 64 ch", objs, tensors

    for build in (lambda: analog(2, 128), lambda: analog(4, 64), spectral):
        name, objs, tensors = build()
        assert all(_resident(o)[0] is t for o, t in zip(objs, tensors))
        plan = K._plan(objs)
        kernel, out = kernel_call(plan, tensors)
        torch_call = lambda: torch.cat(tensors, dim=-1)                        # noqa: E731
        kernel()
        want = torch_call()
        assert want.shape == out.shape and torch.equal(want.view(torch.uint8), out.view(torch.uint8)), name
        del want
        nbytes = 2 * out.numel() * out.element_size()
        res = compare({"operator": lambda: spy.concat(*objs), "kernel": kernel, "torch": torch_call}, args.reps, args.rounds)
        line = dict(case=name, bytes=nbytes, floor_ms=nbytes / HBM_BYTES * 1e3, reps=args.reps, rounds=args.rounds)
        for k, (med, lo, hi) in res.items():
            line[k + "_ms"], line[k + "_min_ms"], line[k + "_max_ms"] = med, lo, hi
            line[k + "_tbyte_per_s"] = nbytes / med * 1e-9
        line["kernel_over_torch"] = res["kernel"][0] / res["torch"][0]
        line["operator_over_torch"] = res["operator"][0] / res["torch"][0]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del out, kernel, objs, tensors, plan
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
