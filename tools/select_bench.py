"""Time spy.selectdata on resident data objects beside torch's own slicing / index_select on the same tensors.

On a float32 AnalogData of 256 channels x 4096 samples x 1000 trials:
  (a) all trials, a latency window of half of each trial   - whole rows, one contiguous run per trial;
  (b) channel=slice(0, 128)                                 - runs of 512 bytes, 16-byte lanes;
  (c) 128 scattered channels                                - element lanes, the index list in LDS;
and on a complex64 SpectralData of (1000, 7, 2049, 64):
  (d) frequency=[30, 60] + taper=[0, 2, 4]                  - a list on a middle axis over runs of 61 x 64 elements.

Per case three figures, each the median over rounds of a window of `reps` calls between two device events (one warm-up
round; the three alternate inside a round, so that they see the same machine): the front end as the user writes it
(planner, row table and launch), the kernel alone (backend.select on a table that is already built), and torch's
`x[...].contiguous()` / `index_select` into a fresh tensor.  Bytes are the ones the selection has to move (read what is
selected, write it) and the rates are those bytes over the time; an MI355X copies at 6.29 TB/s measured
(tools/hbm_rw_probe.hip).  Writes one JSON line per case to profiles/select_bench.jsonl.

    python tools/select_bench.py [--trials 1000] [--reps 10] [--rounds 7]
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
from syncopy_amd.datatype import selectdata as S  # noqa: E402
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


def kernel_call(plan, src):
    """the launch the front end makes for `plan` from the resident tensor, with its table built once"""
    n = np.array([b - a for a, b in plan.rows], dtype=np.int64)
    desc = np.stack([plan.starts, np.array([a for a, _ in plan.rows], dtype=np.int64), n], axis=1)
    out = torch.empty((plan.nrows,) + plan.inner, dtype=src.dtype, device=src.device)
    return lambda: backend.select(src, desc, out, plan.axes), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.jsonl"))
    args = ap.parse_args()
    backend.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(1)
    T = args.trials
    lines = []

    def analog():
        nsamp, nchan = 4096, 256
        starts = np.arange(T) * nsamp
        t = torch.randn((T * nsamp, nchan), generator=gen, device=dev, dtype=torch.float32)
        x = spy.AnalogData(None, samplerate=1000.0)
        x.trialdefinition = np.stack([starts, starts + nsamp, np.full(T, -nsamp // 2)], axis=1)
        x.channel = np.array([f"ch{c}" for c in range(nchan)])
        x.adopt_device_result(t)
        scattered = np.sort(np.random.default_rng(2).permutation(nchan)[:128])
        scat_t = torch.from_numpy(scattered).to(dev)
        kind = f"AnalogData float32 {nchan} ch x {nsamp} x {T} trials"
        q = nsamp // 4
        return x, t, {
            f"{kind}: (a) latency, half of each trial": (
                {"latency": [-q / 1000.0, (q - 1) / 1000.0]}, lambda: t.view(T, nsamp, nchan)[:, q:3 * q].contiguous().view(-1, nchan)),
            f"{kind}: (b) channel=slice(0, 128)": ({"channel": slice(0, 128)}, lambda: t[:, :128].contiguous()),
            f"{kind}: (c) 128 scattered channels": ({"channel": scattered}, lambda: t.index_select(1, scat_t)),
        }

    def spectral():
        shape = (T, 7, 2049, 64)
        t = torch.view_as_complex(torch.randn(shape + (2,), generator=gen, device=dev, dtype=torch.float32))
        s = spy.SpectralData(None, samplerate=2048.0)
        s.trialdefinition = np.stack([np.arange(T), np.arange(T) + 1, np.zeros(T)], axis=1)
        s.freq, s.taper = np.arange(2049) * 0.5, np.array([f"taper{i}" for i in range(7)])
        s.channel = np.array([f"ch{c}" for c in range(64)])
        s.set_pending(lambda: backend.to_host(t), shape, np.complex64)
        s._resident = t
        tapers = torch.tensor([0, 2, 4], device=dev)
        return s, t, {
            f"SpectralData complex64 {T} x 7 x 2049 x 64: (d) frequency=[30, 60] + taper=[0, 2, 4]": (
                {"frequency": [30, 60], "taper": [0, 2, 4]}, lambda: t[:, :, 60:121].index_select(1, tapers)),
        }

    for build in (analog, spectral):
        obj, src, cases = build()
        assert _resident(obj)[0] is src
        for name, (kwargs, torch_call) in cases.items():
            plan = S._plan(obj, **kwargs)
            kernel, out = kernel_call(plan, src)
            kernel()
            want = torch_call()
            assert want.shape == out.shape and torch.equal(want.view(torch.uint8), out.view(torch.uint8)), name
            del want
            nbytes = 2 * out.numel() * out.element_size()
            res = compare({"operator": lambda: spy.selectdata(obj, **kwargs), "kernel": kernel, "torch": torch_call},
                          args.reps, args.rounds)
            line = dict(case=name, bytes=nbytes, floor_ms=nbytes / HBM_BYTES * 1e3, reps=args.reps, rounds=args.rounds)
            for k, (med, lo, hi) in res.items():
                line[k + "_ms"], line[k + "_min_ms"], line[k + "_max_ms"] = med, lo, hi
                line[k + "_tbyte_per_s"] = nbytes / med * 1e-9
            line["kernel_over_torch"] = res["kernel"][0] / res["torch"][0]
            line["operator_over_torch"] = res["operator"][0] / res["torch"][0]
            print(json.dumps(line), flush=True)
            lines.append(line)
            del out, kernel
        del obj, src, cases
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
