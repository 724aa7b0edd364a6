"""A hash of the output bytes of the wavelet transform over a fixed seeded matrix of plans, through the public CWTPlan API
only: two builds of the library that launch the same kernels over the same ranges in the same order write the same file,
byte for byte (the transform has no atomics and sums in a fixed order).

    PYTHONPATH=. python tools/cwt_route_dump.py OUT.json
"""
import hashlib
import json
import sys

import numpy as np
import torch

from syncopy_amd import backend as be

DT = 1e-3


def morlet_scales(freqs):
    return (6 + np.sqrt(38)) / (4 * np.pi * np.asarray(freqs, dtype=np.float64))


# the pinned plans of tests/test_cwt_route.py: (samples, frequencies in Hz, channels)
PLANS = {"two_direct_one_staged": (3000, [8, 30, 45, 70, 95], 3), "own_sum_set": (4500, [24, 40, 64, 100], 3),
         "pieces": (20000, [0.3, 0.5, 1.5, 20], 3), "sum_falls_back": (4500, [0.9, 1.6, 20], 3)}


def trials(nsig, nchan, T, seed):
    g = torch.Generator().manual_seed(seed)
    data = (torch.randn((T * nsig + 16, nchan), generator=g, dtype=torch.float32) + 0.75).cuda()
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig + 8
    return data, st


def record(res, tag, out):
    torch.cuda.synchronize()
    res[tag] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def run(res, tag, nsig, scales, nchan, T=3, output="pow", detrend=0, direct=True, precision64=False, accumulate=(0, 1, 2), **kw):
    """Per-segment outputs, out[b] += segment b on top of them, and the trial sum in split calls of T - 1 and 1 trials."""
    data, st = trials(nsig, nchan, T, 1000 * nsig + nchan + T)
    plan = be.CWTPlan(nsig, nchan, scales, DT, 6.0, detrend, output, **kw)
    if not direct:
        plan.set_direct(False)
    if precision64:
        assert plan.set_precision(True)
    lo, hi = st - 8, st + nsig + 8                         # the trial runs past the selected samples on both sides
    each = None
    if 0 in accumulate:
        each = plan.execute(data, st, lo, hi)
        record(res, tag + "_each", each)
    if 1 in accumulate:
        acc = each.clone() if each is not None else torch.zeros(plan.out_shape(T), dtype=plan.out_dtype, device="cuda")
        record(res, tag + "_add", plan.execute(data, st, lo, hi, out=acc, accumulate=1))
    if 2 in accumulate:
        total = torch.zeros(plan.out_shape(1), dtype=plan.out_dtype, device="cuda")
        for a, b in ((0, T - 1), (T - 1, T)):
            if b > a:
                plan.execute(data, st[a:b].contiguous(), lo[a:b].contiguous(), hi[a:b].contiguous(), out=total, accumulate=2)
        record(res, tag + "_sum", total)


def main():
    be.require_gpu()
    res = {}
    for name, (nsig, freqs, nchan) in PLANS.items():
        sc = morlet_scales(freqs)
        for output in ("pow", "fourier"):
            run(res, f"{name}_{output}", nsig, sc, nchan, output=output)
        run(res, f"{name}_staged", nsig, sc, nchan, direct=False, accumulate=(0, 2))
    nsig, freqs, nchan = PLANS["two_direct_one_staged"]
    sc = morlet_scales(freqs)
    for output in ("abs", "real", "imag", "angle", "absreal", "absimag"):                  # every output kind
        run(res, f"kind_{output}", nsig, sc, nchan, output=output, accumulate=(0,))
    for detrend in (None, 1):                                                             # (0: every other case)
        run(res, f"detrend_{detrend}", nsig, sc, nchan, detrend=detrend, accumulate=(0,))
    run(res, "one_channel", nsig, sc, 1)                                                  # no channel-major input copy
    run(res, "odd_trials", nsig, sc, 5, T=5)                                              # a half-empty last pair
    keep = np.unique(np.r_[0:5, 3:2900:7, 1023, 1024, 2047, 2048, 2999])
    tpos = np.full(nsig, -1, dtype=np.int32)
    tpos[keep] = np.arange(keep.size)
    run(res, "selected_samples", nsig, sc, nchan, tpos=tpos, ntime_out=keep.size)
    run(res, "gapped_slots", nsig, sc, nchan, tpos=(7 * np.arange(nsig) + 3).astype(np.int32), ntime_out=7 * nsig + 5,
        accumulate=(0, 1))
    run(res, "slots_not_increasing", nsig, sc, nchan, tpos=np.r_[1, 0, 2:nsig].astype(np.int32), ntime_out=nsig, accumulate=(0,))
    small = [0.05, 0.012, 0.004]
    run(res, "family_MorletSL", 1400, np.array(small) / 3.0, nchan, output="fourier", sl_cycles=3.0, accumulate=(0,))
    run(res, "family_Paul4", 1400, small, nchan, output="fourier", family="Paul", order=4, accumulate=(0,))
    run(res, "family_DOG2", 1400, small, nchan, output="fourier", family="DOG", order=2, accumulate=(0,))
    run(res, "family_DOG6", 1400, small, nchan, output="abs", family="DOG", order=6, accumulate=(0,))
    run(res, "float64", 1400, small, nchan, output="fourier", precision64=True)
    run(res, "c4_shape", 16384, morlet_scales(np.arange(4, 101, 4)), 128, T=4)            # the benchmark's wavelet case
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(len(res), "cases ->", sys.argv[1])


if __name__ == "__main__":
    main()
