"""Time the device route of spy.synthdata and say where the time goes.

  (a) ar2_network, 64 channels coupled by mk_RandomAdjMat, 4096 samples x 200 trials, beside the host path (the
      reference's loop of one matrix-vector product per sample, unchanged by the device route) on 8 trials;
  (b) the uncoupled network, 256 channels x 4096 samples x 1000 trials, beside ar2_uncoupled_fast (a torch loop of
      3 x 4096 launches with the device's own random stream);
  (c) phase_diffusion and harmonic at 256 x 4096 x 1000.

Per case: the front end as the user calls it (wall clock, device idle before and after), and its parts on the same
chunks - the host's draw of the noise (up to 16 threads), the upload, and the kernel between two device events (per chunk
the median of `--reps` launches after one warm-up launch, summed over the chunks).  The host path beside case (a) is
this commit's, whose trial loop (`synthdata._ar2_trial`) does what it did before the device route.  One JSON line per case goes
to --out.  Run one case per process:

    python tools/synth_bench.py --case a [--out profiles/synth_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import syncopy_amd as spy  # noqa: E402
from syncopy_amd import backend  # noqa: E402

S = spy.synthdata


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def parts(kind, nTrials, nSamples, nChannels, seed, reps, launch):
    """host draw, upload and kernel seconds, each summed over the chunks the front end makes (the kernel of a chunk: the
    median of `reps` launches); launch(noise_d, rows, k0, k1) queues the kernel of the trials [k0, k1)"""
    dtype = np.float64 if kind == "ar2" else np.float32
    seeds = S._trial_seeds(seed, nTrials)
    res = torch.empty((nTrials * nSamples, nChannels), dtype=torch.float32, device="cuda")
    draw = up = kern = 0.0
    chunks = S._trial_chunks(nTrials, nSamples * nChannels * np.dtype(dtype).itemsize, S.CHUNK_BYTES)
    for k0, k1 in chunks:
        t0 = time.perf_counter()
        noise = torch.from_numpy(S.draw_noise(seeds[k0:k1], nSamples, nChannels, dtype))
        draw += time.perf_counter() - t0
        dt, noise_d = wall(lambda: noise.to("cuda"))
        up += dt
        rows = res[k0 * nSamples:k1 * nSamples]
        kern += kernel_ms(lambda: launch(noise_d, rows, k0, k1), reps) * 1e-3
    return dict(chunks=len(chunks), host_draw_s=draw, upload_s=up, kernel_s=kern)


def report(name, shape, front_s, p, extra):
    total = p["host_draw_s"] + p["upload_s"] + p["kernel_s"]
    row = dict(case=name, channels=shape[0], samples=shape[1], trials=shape[2], front_end_s=front_s, **p,
               host_draw_share=p["host_draw_s"] / total, kernel_ms_per_trial=1e3 * p["kernel_s"] / shape[2],
               front_end_ms_per_trial=1e3 * front_s / shape[2], **extra)
    print(json.dumps(row), flush=True)
    return row


def case_a(reps):
    C, N, T = 64, 4096, 200
    adj = S.mk_RandomAdjMat(C, seed=1)
    kw = dict(AdjMat=adj, nSamples=N, seed=5)
    S.ar2_network(nTrials=2, device=True, **kw)                     # (library and context loaded)
    front, _ = wall(lambda: S.ar2_network(nTrials=T, device=True, **kw))
    table = backend.synth_table(*S.coupling_table(adj), torch.device("cuda", 0))
    p = parts("ar2", T, N, C, 5, reps, lambda nz, rows, k0, k1: backend.synth_ar2(nz, 0.55, -0.8, table, rows))
    t0 = time.perf_counter()
    S.ar2_network(nTrials=8, **kw)
    host = (time.perf_counter() - t0) / 8
    return report("a: ar2_network coupled", (C, N, T), front, p,
                  dict(couplings=int(table[0][-1]), host_path_ms_per_trial=1e3 * host, host_path_trials=8,
                       speedup_per_trial=host / (front / T)))


def case_b(reps):
    C, N, T = 256, 4096, 1000
    kw = dict(AdjMat=np.zeros((C, C)), nSamples=N, seed=5)
    S.ar2_network(nTrials=2, device=True, **kw)
    front, _ = wall(lambda: S.ar2_network(nTrials=T, device=True, **kw))
    table = backend.synth_table(*S.coupling_table(np.zeros((C, C))), torch.device("cuda", 0))
    p = parts("ar2", T, N, C, 5, reps, lambda nz, rows, k0, k1: backend.synth_ar2(nz, 0.55, -0.8, table, rows))
    S.ar2_uncoupled_fast(C, 64, 4, seed=1)
    fast, _ = wall(lambda: S.ar2_uncoupled_fast(C, N, T, seed=1))
    return report("b: ar2_network uncoupled", (C, N, T), front, p, dict(ar2_uncoupled_fast_s=fast))


def case_c(reps):
    C, N, T = 256, 4096, 1000
    rows_out = []
    S.phase_diffusion(60, nSamples=N, nChannels=C, nTrials=2, seed=5, device=True)
    front, _ = wall(lambda: S.phase_diffusion(60, nSamples=N, nChannels=C, nTrials=T, seed=5, device=True))
    lin, _, rel = S._phase_tables(60, 0.1, 1000, C, N, False, None)
    lin_d = torch.from_numpy(lin).cuda()

    def launch(wn, rows, k0, k1):
        backend.synth_phase(wn, lin_d, torch.zeros((k1 - k0, C), dtype=torch.float32, device="cuda"), float(rel), True, rows)
    rows_out.append(report("c: phase_diffusion", (C, N, T), front, parts("phase", T, N, C, 5, reps, launch), {}))
    S.harmonic(30, nSamples=N, nChannels=C, nTrials=2, device=True)
    front, _ = wall(lambda: S.harmonic(30, nSamples=N, nChannels=C, nTrials=T, device=True))
    col = torch.from_numpy(S._harmonic_column(30, 1000, N)).cuda()
    out = torch.empty((T * N, C), dtype=torch.float32, device="cuda")
    ms = kernel_ms(lambda: backend.synth_tile(col, T, out), reps)
    row = dict(case="c: harmonic", channels=C, samples=N, trials=T, front_end_s=front, kernel_s=ms * 1e-3,
               kernel_tb_per_s=out.numel() * 4 / (ms * 1e-3) / 1e12, host_draw_share=0.0)
    print(json.dumps(row), flush=True)
    rows_out.append(row)
    return rows_out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("a", "b", "c"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_bench.jsonl"))
    args = ap.parse_args()
    result = {"a": case_a, "b": case_b, "c": case_c}[args.case](args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for row in result if isinstance(result, list) else [result]:
            fh.write(json.dumps(row) + "\n")
