"""Hashes of what the Wilson / Granger stage (K6) returns over a fixed seeded matrix of shapes and entry points: two builds of
the library that launch the same kernels over the same data in the same order write the same file, byte for byte (the
kernels are deterministic: fixed-order reductions, no atomics).

    PYTHONPATH=. python tools/granger_route_dump.py OUT.json

With a kernel trace of such a run (rocprofv3 --kernel-trace, CSV output),

    python tools/granger_route_dump.py --condense KERNEL_TRACE.csv OUT.txt

writes the launches in order as "kernel grid", repeated blocks (the iterations) folded into "N x { ... }".
"""
import csv
import hashlib
import json
import sys

import numpy as np

# the list N of tests/test_gpu_wilson_kernels.py (every size class from 48 up) and two sizes below the matrix-core products
N = [48, 63, 65, 100, 128, 161, 200, 255, 257, 300, 16, 33]
NFREQ = [33, 65]
UNCONVERGED = [(70, 129, 25), (100, 65, 20)]          # test_unconverged_error_is_over_all_bins: n, F, seed; 10 iterations
PLUS = [(18, 9), (33, 9), (129, 9), (2049, 9), (4097, 9), (2501, 9), (3001, 9), (8193, 9), (8193, 2116)]      # test_plus_operator


def var_csd(C, F, seed, floor=0.05):
    """S(f) = H(f) Sigma H(f)^H + floor of a random stable VAR(2) process (the fixture of tests/test_gpu_wilson_kernels.py)."""
    rng = np.random.default_rng(seed)
    A1 = 0.5 * np.eye(C) + rng.normal(size=(C, C)) * (0.25 / np.sqrt(C))
    A2 = -0.6 * np.eye(C) + rng.normal(size=(C, C)) * (0.15 / np.sqrt(C))
    L = np.eye(C) + 0.1 * np.tril(rng.normal(size=(C, C)), -1)
    Sigma = L @ L.T
    w = np.pi * np.arange(F) / (F - 1)
    A = np.eye(C)[None] - A1[None] * np.exp(-1j * w)[:, None, None] - A2[None] * np.exp(-2j * w)[:, None, None]
    H = np.linalg.inv(A)
    S = H @ Sigma[None] @ H.conj().transpose(0, 2, 1) + floor * np.eye(C)[None]
    return 0.5 * (S + S.conj().transpose(0, 2, 1))


def unconverged_csd(n, F, seed):
    """A rank-1 PSD block cancels all but 1e-6 of entry (5, 7) of bin 13, which no subset of every 8th bin holds."""
    csd = var_csd(n, F, seed)
    a, b = 5, 7
    s = csd[13, a, b] * (1.0 - 1e-6)
    csd[13, a, a] += abs(s)
    csd[13, b, b] += abs(s)
    csd[13, a, b] -= s
    csd[13, b, a] -= np.conj(s)
    return csd


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def dump(path):
    import torch
    from syncopy_amd import backend as be
    from syncopy_amd.connectivity.wilson_sharded import HipPrims, granger_sharded
    be.require_gpu()
    prims = HipPrims()
    res = {}

    cases = [(f"n{n}_F{F}", var_csd(n, F, seed=n), 100) for n in N for F in NFREQ]
    cases += [(f"n{n}_F{F}_unconverged", unconverged_csd(n, F, seed), 10) for n, F, seed in UNCONVERGED]
    cases = [(tag, torch.from_numpy(np.ascontiguousarray(csd.astype(np.complex64))).cuda(), niter) for tag, csd, niter in cases]

    def record(tag, G, meta, H, S, iterations):
        info = [float(meta["converged"]), meta["max rel. err"], float(meta["reg. factor"]), meta["initial cond. num"]]
        res[tag] = [digest(G), digest(H), digest(S), [float(v).hex() for v in info], iterations]

    # every case through spyhip_granger, then every case through the stepped entry points with one shard, then the plus
    # operator alone: three contiguous parts of a kernel trace
    for tag, dev, niter in cases:
        G, meta, H, S = be.granger(dev, niter=niter, want_factors=True)
        record(tag + "_granger", G, meta, H, S, be.granger_stats()["iterations"])
    for tag, dev, niter in cases:
        G, meta, H, S = granger_sharded(dev, 0, dev.shape[0], prims, niter=niter)
        record(tag + "_stepped", G, meta, H, S, meta["iterations"])
    for nftot, nent in PLUS:
        rng = np.random.default_rng(nftot + nent)
        g = rng.normal(size=(nftot, nent)) + 1j * rng.normal(size=(nftot, nent))
        gp, g0 = prims.plus(torch.from_numpy(g).cuda())
        res[f"plus_F{nftot}_E{nent}"] = [digest(gp), digest(g0)]
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(len(res), "cases ->", path)


def fold(seq, max_period=64):
    """Greedy run-length folding of repeated blocks of at most max_period lines."""
    out, i = [], 0
    while i < len(seq):
        best = (1, 1)
        for p in range(1, min(max_period, (len(seq) - i) // 2) + 1):
            reps = 1
            while seq[i + reps * p:i + (reps + 1) * p] == seq[i:i + p]:
                reps += 1
            if reps > 1 and reps * p > best[0] * best[1]:
                best = (p, reps)
        p, reps = best
        if reps == 1:
            out.append(seq[i])
        else:
            out.append(f"{reps} x {{")
            out.extend("    " + s for s in fold(seq[i:i + p], max_period))
            out.append("}")
        i += p * reps
    return out


def condense(src, dst):
    with open(src, newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    grid = lambda r: "x".join(str(int(r[f"Grid_Size_{a}"]) // max(int(r[f"Workgroup_Size_{a}"]), 1)) for a in "XYZ")
    seq = [f'{r["Kernel_Name"].split("(")[0]} {grid(r)}' for r in rows if "spywil" in r["Kernel_Name"]]
    with open(dst, "w") as fh:
        fh.write(f"{len(seq)} launches of K6 kernels, in order: kernel, workgroups\n")
        fh.write("\n".join(fold(seq)) + "\n")
    print(len(seq), "launches ->", dst)


if __name__ == "__main__":
    if sys.argv[1] == "--condense":
        condense(sys.argv[2], sys.argv[3])
    else:
        dump(sys.argv[1])
