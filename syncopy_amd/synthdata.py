"""Synthetic data generators with the reference's sampling scheme (syncopy/synthdata/analog.py and the per-trial seeding
of syncopy/synthdata/utils.py: collect_trials), used for tutorials, parity fixtures and the benchmark inputs;
`poisson_noise` is the SpikeData generator of syncopy/synthdata/spikes.py.

Every trial generator (`white_noise`, `linear_trend`, `harmonic`, `phase_diffusion`, `ar2_network`, `red_noise`) takes the
keywords of the reference's `collect_trials`: `nTrials` (None: the single trial as an ndarray), `samplerate`, `seed` and
`seed_per_trial` (True: trial k gets `default_rng(seed).integers(1_000_000, size=nTrials)[k]`; False: every trial gets
`seed`), and like there a `cfg` dictionary may carry any of the keywords (`harmonic(cfg)`, `harmonic(cfg=cfg)`).  The
host path is NumPy only and DEFINES every result: every random number comes from `np.random.default_rng`.

Deviations from the reference, on purpose:
  * `device=` (not in the reference; default False).  `device=True` needs `nTrials` and a gfx950 device and returns an
    AnalogData whose data is resident on the device (the host copy is fetched when `.data` is first read), so that
    `2 * harmonic(..., device=True) + white_noise(..., device=True)` never leaves it.  The random numbers are still the
    host's: each trial's noise is one `default_rng(trial_seed).normal(size=(nSamples, nChannels))` (the very stream of the
    reference's row-by-row draws), drawn by up to 16 threads and uploaded in trial chunks of at most CHUNK_BYTES.  Only the
    deterministic part runs on the device (csrc/synth.hip): the AR(2) recursion, the cumulative phase, the tiling.  The
    tiling, the phase and the uncoupled AR(2) recursion give the host's bits; the coupled recursion sums its float64
    products in ascending sender order, not in the BLAS's, which can flip a float32 rounding; the
    cosine of `phase_diffusion` is the device's cosf.
  * The dtypes are pinned to what the reference gives under NumPy 1 (value-based casting), under which it was written
    and its goldens made: `phase_diffusion` is float32 throughout - the float64 scalar sqrt(omega0 / samplerate * eps) is
    cast to float32 when it multiplies the float32 noise, and the cumulative sum, the phase and the cosine are float32.
    The same text run under NumPy 2 yields float64; the casts here are explicit, so the result does not depend on the
    installed NumPy.  For the same reason the lag-2 parameter of `ar2_network` multiplies the float32 signal as a float32
    (also when `alphas` holds NumPy float64 scalars), which is what the device computes.
  * The device route of `ar2_network` and `red_noise` takes at most 1024 channels (one thread per channel in one
    workgroup).
  * `ar2_uncoupled_fast` is not the reference's random stream at all (benchmark inputs only).
"""
import numpy as np

from .datatype import AnalogData, SpikeData
from .shared.kwarg_decorators import unwrap_cfg

# bytes of host noise that are on their way to the device at once
CHUNK_BYTES = 512 << 20
# threads that draw the trials' noise (a fixed bound: the machine's CPU count says nothing about this process's share)
DRAW_THREADS = 16
# channels of the device route of the AR(2) generators (csrc/synth_route.h: MAX_CHAN)
MAX_DEVICE_CHANNELS = 1024


def _trial_seeds(seed, nTrials, seed_per_trial=True):
    if seed is None or not seed_per_trial:
        return [seed] * nTrials
    return list(np.random.default_rng(seed).integers(1_000_000, size=nTrials))


def _check_trials(nTrials):
    if isinstance(nTrials, bool) or not isinstance(nTrials, (int, np.integer)) or nTrials < 1:
        raise ValueError(f"nTrials must be an integer >= 1 or None, not {nTrials!r}")


def _ar2_trial(AdjMat, nSamples, alphas, seed):
    AdjMat = np.asarray(AdjMat).astype(np.float32)
    nChannels = AdjMat.shape[0]
    alpha1, alpha2 = alphas
    # what NumPy 1 makes of any scalar that meets the float32 signal; under NumPy 2 a Python float gives the same bits,
    # a float64 scalar would not
    alpha2 = np.float32(alpha2)
    M = np.diag(nChannels * [alpha1]) + AdjMat.T
    sig = np.zeros((nSamples, nChannels), dtype=np.float32)
    rng = np.random.default_rng(seed)
    sig[:2, :] = rng.normal(size=(2, nChannels))
    for i in range(2, nSamples):
        sig[i, :] = M @ sig[i - 1, :] + alpha2 * sig[i - 2, :]
        sig[i, :] += rng.normal(size=nChannels)
    return sig


def _white_noise_trial(nSamples, nChannels, seed):
    return np.random.default_rng(seed).normal(size=(nSamples, nChannels)).astype("f4")


def _trend_column(y_max, nSamples):
    return np.linspace(0, y_max, nSamples, dtype="f4")


def _harmonic_column(freq, samplerate, nSamples):
    tvec = np.arange(nSamples) * 1 / samplerate
    return np.cos(2 * np.pi * freq * tvec, dtype="f4")


def _initial_phases(nChannels, seed):
    """the random initial phases of one trial of phase_diffusion: the second stream of its seed, float32"""
    return np.float32(2 * np.pi) * np.random.default_rng(seed).uniform(size=nChannels).astype("f4")


def _phase_tables(freq, eps, samplerate, nChannels, nSamples, rand_ini, seed):
    """(float32 linear phase omega0 * tvec (nSamples), float32 initial phases (nChannels), float64 scale of the Brownian
    increments) of one trial of phase_diffusion, in NumPy-1 dtypes"""
    tvec = np.linspace(0, nSamples / samplerate, nSamples, dtype="f4")
    omega0 = 2 * np.pi * freq
    lin = np.float32(omega0) * tvec
    ps0 = _initial_phases(nChannels, seed) if rand_ini else np.zeros(nChannels, dtype="f4")
    return lin, ps0, np.sqrt(omega0 / samplerate * eps)


def _phase_diffusion_trial(freq, eps, samplerate, nChannels, nSamples, rand_ini, return_phase, seed):
    wn = _white_noise_trial(nSamples, nChannels, seed)
    lin, ps0, rel_eps = _phase_tables(freq, eps, samplerate, nChannels, nSamples, rand_ini, seed)
    lin_phase = np.tile(lin, (nChannels, 1)).T
    if rand_ini:
        lin_phase += ps0
    brown_incr = np.float32(rel_eps) * wn
    phases = lin_phase + np.cumsum(brown_incr, axis=0, dtype="f4")
    return phases if return_phase else np.cos(phases)


def _default_adjmat():
    AdjMat = np.zeros((2, 2), dtype=np.float32)
    AdjMat[1, 0] = 0.25
    return AdjMat


def coupling_table(AdjMat):
    """(rowptr int32 (n + 1), col int32, w float32): the non-zeros of AdjMat.T (float32) as CSR - receiver c has the
    senders col[rowptr[c]:rowptr[c + 1]], ascending, with the weights w (include/spyhip.h: spyhip_synth_ar2)"""
    M = np.asarray(AdjMat).astype(np.float32).T
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 1:
        raise ValueError("AdjMat must be a square matrix")
    rows, cols = np.nonzero(M)                                   # C-order: row by row, columns ascending
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=M.shape[0])))).astype(np.int32)
    return rowptr, np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(M[rows, cols], dtype=np.float32)


# ---- the trial generators ---------------------------------------------------------------------------------------------
@unwrap_cfg
def white_noise(nSamples=1000, nChannels=2, seed=None, nTrials=100, samplerate=1000, seed_per_trial=True, device=False):
    """White noise of unit variance, float32."""
    if device:
        return _on_device("white", nTrials, samplerate, seed, seed_per_trial, nSamples, nChannels)
    if nTrials is None:
        return _white_noise_trial(nSamples, nChannels, seed)
    _check_trials(nTrials)
    return _collect([_white_noise_trial(nSamples, nChannels, s) for s in _trial_seeds(seed, nTrials, seed_per_trial)],
                    samplerate)


@unwrap_cfg
def linear_trend(y_max, nSamples=1000, nChannels=2, nTrials=100, samplerate=1000, seed=None, seed_per_trial=True,
                 device=False):
    """A linear trend from 0 to `y_max` over the trial, on every channel (`seed` has nothing to act on)."""
    col = _trend_column(y_max, nSamples)
    if device:
        return _on_device("tile", nTrials, samplerate, None, True, nSamples, nChannels, col=col)
    trial = np.column_stack([col for _ in range(nChannels)])
    if nTrials is None:
        return trial
    _check_trials(nTrials)
    return _collect([trial] * nTrials, samplerate)


@unwrap_cfg
def harmonic(freq, samplerate=1000, nSamples=1000, nChannels=2, nTrials=100, seed=None, seed_per_trial=True, device=False):
    """cos(2 pi freq t) on every channel (`seed` has nothing to act on)."""
    col = _harmonic_column(freq, samplerate, nSamples)
    if device:
        return _on_device("tile", nTrials, samplerate, None, True, nSamples, nChannels, col=col)
    trial = np.column_stack([col for _ in range(nChannels)])
    if nTrials is None:
        return trial
    _check_trials(nTrials)
    return _collect([trial] * nTrials, samplerate)


@unwrap_cfg
def phase_diffusion(freq, eps=0.1, samplerate=1000, nChannels=2, nSamples=1000, rand_ini=False, return_phase=False,
                    seed=None, nTrials=100, seed_per_trial=True, device=False):
    """Linear phase evolution 2 pi freq t plus a Brownian term whose increments are `eps` relative to the linear ones;
    the cosine of the phase, or with `return_phase` the phase itself.  `rand_ini`: random initial phases.  float32."""
    if device:
        return _on_device("phase", nTrials, samplerate, seed, seed_per_trial, nSamples, nChannels,
                          phase=(freq, eps, rand_ini, return_phase))
    if nTrials is None:
        return _phase_diffusion_trial(freq, eps, samplerate, nChannels, nSamples, rand_ini, return_phase, seed)
    _check_trials(nTrials)
    return _collect([_phase_diffusion_trial(freq, eps, samplerate, nChannels, nSamples, rand_ini, return_phase, s)
                     for s in _trial_seeds(seed, nTrials, seed_per_trial)], samplerate)


@unwrap_cfg
def ar2_network(AdjMat=None, nSamples=1000, alphas=(0.55, -0.8), seed=None, nTrials=100, samplerate=1000,
                seed_per_trial=True, device=False):
    """Network of coupled AR(2) processes; entry (i, j) of `AdjMat` couples i -> j."""
    if AdjMat is None:
        AdjMat = _default_adjmat()
    if device:
        return _on_device("ar2", nTrials, samplerate, seed, seed_per_trial, nSamples, np.asarray(AdjMat).shape[0],
                          ar2=(AdjMat, alphas))
    if nTrials is None:
        return _ar2_trial(AdjMat, nSamples, alphas, seed)
    _check_trials(nTrials)
    trials = [_ar2_trial(AdjMat, nSamples, alphas, s) for s in _trial_seeds(seed, nTrials, seed_per_trial)]
    return _collect(trials, samplerate)


@unwrap_cfg
def red_noise(alpha, nSamples=1000, nChannels=2, seed=None, nTrials=100, samplerate=1000, seed_per_trial=True,
              device=False):
    """Uncoupled AR(1) processes x[i] = alpha x[i-1] + noise, `alpha` in [0, 1): `ar2_network` with alphas = [alpha, 0]
    and no coupling."""
    return ar2_network(AdjMat=np.diag(np.zeros(nChannels)), nSamples=nSamples, alphas=[alpha, 0], seed=seed,
                       nTrials=nTrials, samplerate=samplerate, seed_per_trial=seed_per_trial, device=device)


def ar2_peak_freq(a1, a2, samplerate=1):
    """The frequency of the spectral peak of an AR(2) process with the lag-1 and lag-2 parameters `a1`, `a2`."""
    if np.any((a1 ** 2 + 4 * a2) > 0):
        raise ValueError("No complex roots!")
    return np.arccos(a1 * (a2 - 1) / (4 * a2)) * 1 / (np.pi * 2) * samplerate


def mk_RandomAdjMat(nChannels=3, conn_thresh=0.25, max_coupling=0.25, seed=None):
    """A random adjacency matrix for `ar2_network`: entry (i, j), the coupling i -> j, exists with probability
    `conn_thresh` (never on the diagonal), and the couplings into one channel add up to `max_coupling`."""
    AdjMat = (np.random.default_rng(seed).random((nChannels, nChannels)) < conn_thresh).astype(float)
    np.fill_diagonal(AdjMat, 0)
    norm = AdjMat.sum(axis=0)
    norm[norm == 0] = 1
    return AdjMat / norm[None, :] * max_coupling


def _trialdefinition(nTrials, nSamples, samplerate):
    starts = np.arange(nTrials) * nSamples
    return np.stack([starts, starts + nSamples, np.full(nTrials, -samplerate)], axis=1)


def _collect(trials, samplerate):
    """Trials stacked along time; like the reference's generator-built AnalogData every trial
    gets a trigger offset of -1 s (time axis starts at -1.0)."""
    n = trials[0].shape[0]
    starts = np.arange(len(trials)) * n
    trl = np.stack([starts, starts + n, np.full(len(trials), -samplerate)], axis=1)
    return AnalogData(np.concatenate(trials, axis=0), samplerate=samplerate, trialdefinition=trl)


# ---- the device route ---------------------------------------------------------------------------------------------------
def draw_noise(seeds, nSamples, nChannels, dtype):
    """(len(seeds), nSamples, nChannels): trial k is default_rng(seeds[k]).normal(size=(nSamples, nChannels)) as `dtype`,
    drawn by up to DRAW_THREADS threads (the generator releases the interpreter lock while it fills)."""
    from concurrent.futures import ThreadPoolExecutor
    out = np.empty((len(seeds), nSamples, nChannels), dtype=dtype)

    def one(k):
        out[k] = np.random.default_rng(seeds[k]).normal(size=(nSamples, nChannels))
    if len(seeds) == 1:
        one(0)
        return out
    with ThreadPoolExecutor(max_workers=min(DRAW_THREADS, len(seeds))) as pool:
        list(pool.map(one, range(len(seeds))))
    return out


def _trial_chunks(nTrials, trial_bytes, nbytes):
    """[k0, k1) trial ranges of at most `nbytes` (at least one trial each)"""
    per = max(1, int(nbytes) // max(1, int(trial_bytes)))
    return [(k, min(k + per, nTrials)) for k in range(0, nTrials, per)]


def _on_device(kind, nTrials, samplerate, seed, seed_per_trial, nSamples, nChannels, col=None, phase=None, ar2=None):
    import torch
    from . import backend
    if nTrials is None:
        raise ValueError("device=True returns an AnalogData object: nTrials must be given")
    _check_trials(nTrials)
    nTrials, nSamples, nChannels = int(nTrials), int(nSamples), int(nChannels)
    if nSamples < 1 or nChannels < 1:
        raise ValueError("nSamples and nChannels must be at least 1")
    backend.require_gpu()
    device = torch.device("cuda", torch.cuda.current_device())
    res = torch.empty((nTrials * nSamples, nChannels), dtype=torch.float32, device=device)
    seeds = _trial_seeds(seed, nTrials, seed_per_trial)
    if kind == "tile":
        backend.synth_tile(torch.from_numpy(np.ascontiguousarray(col, dtype=np.float32)).to(device), nTrials, res)
    else:
        if kind == "ar2":
            AdjMat, (alpha1, alpha2) = ar2
            if nSamples < 2:
                raise ValueError("ar2_network needs at least 2 samples")
            if nChannels > MAX_DEVICE_CHANNELS:
                raise ValueError(f"device=True takes at most {MAX_DEVICE_CHANNELS} channels, not {nChannels}")
            table = backend.synth_table(*coupling_table(AdjMat), device)
        elif kind == "phase":
            freq, eps, rand_ini, return_phase = phase
            lin, _, rel_eps = _phase_tables(freq, eps, samplerate, nChannels, nSamples, False, None)
            lin_d = torch.from_numpy(lin).to(device)
        noise_dtype = np.float64 if kind == "ar2" else np.float32
        trial_bytes = nSamples * nChannels * np.dtype(noise_dtype).itemsize
        for k0, k1 in _trial_chunks(nTrials, trial_bytes, CHUNK_BYTES):
            rows = res[k0 * nSamples:k1 * nSamples]
            noise = torch.from_numpy(draw_noise(seeds[k0:k1], nSamples, nChannels, noise_dtype))
            if kind == "white":
                rows.copy_(noise.reshape(-1, nChannels))
                continue
            noise = noise.to(device)
            if kind == "ar2":
                backend.synth_ar2(noise, float(alpha1), float(alpha2), table, rows)
            else:
                ps0 = np.zeros((k1 - k0, nChannels), dtype=np.float32)
                if rand_ini:                                      # every trial's seed draws its own initial phases
                    ps0 = np.stack([_initial_phases(nChannels, s) for s in seeds[k0:k1]])
                backend.synth_phase(noise, lin_d, torch.from_numpy(ps0).to(device), float(rel_eps), not return_phase, rows)
    out = AnalogData(None, samplerate=samplerate)
    out.trialdefinition = _trialdefinition(nTrials, nSamples, samplerate)
    out.adopt_device_result(res)
    out.channel = np.array(["channel" + str(i + 1).zfill(len(str(nChannels))) for i in range(nChannels)])
    return out


def ar2_uncoupled_fast(nChannels, nSamples, nTrials, alphas=(0.55, -0.8), seed=0, samplerate=1000, device=None):
    """Uncoupled AR(2) noise for large benchmark inputs, generated on the GPU (same process
    parameters as ar2_network with AdjMat = 0; not the reference's random stream)."""
    import torch
    dev = torch.device("cuda" if device is None else device)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    a1, a2 = alphas
    x = torch.empty((nTrials, nSamples, nChannels), dtype=torch.float32, device=dev)
    x[:, :2] = torch.randn((nTrials, 2, nChannels), generator=g, device=dev)
    for i in range(2, nSamples):
        x[:, i] = a1 * x[:, i - 1] + a2 * x[:, i - 2] + torch.randn((nTrials, nChannels), generator=g, device=dev)
    return x.reshape(nTrials * nSamples, nChannels)


def poisson_noise(nTrials=10, nSpikes=10000, nChannels=3, nUnits=10, intensity=0.1, samplerate=10000, seed=None):
    """Poisson (shot) noise as SpikeData: `nSpikes` spikes over all trials at `intensity` spikes per sample, so a trial is
    about nSpikes / (intensity * nTrials) samples long.  Trials are shortened by up to 10 % of that, the trigger offsets
    lie between 5 % and 20 % of the shortest trial before its start, and channels and units get uniformly random
    weights.  Signature, order of the draws from default_rng(seed) and hence spikes and trial definition for a seed are
    those of syncopy/synthdata/spikes.py: poisson_noise."""
    def get_rdm_weights(size):
        pvec = np.random.default_rng(seed).uniform(size=size)
        return pvec / pvec.sum()

    rng = np.random.default_rng(seed)
    T_max = int(nSpikes / intensity)                    # total length of all trials combined
    # (choice over the integer T_max draws what choice over range(T_max) draws, without building the list)
    spike_samples = np.sort(rng.choice(T_max, size=nSpikes, replace=False))
    channels = rng.choice(np.arange(nChannels), p=get_rdm_weights(nChannels), size=nSpikes, replace=True)
    units = rng.choice(np.arange(nUnits), p=get_rdm_weights(nUnits), size=nSpikes, replace=True)

    step = T_max // nTrials
    trl_intervals = np.arange(T_max + 1, step=step)
    idx_start = trl_intervals[:-1]
    idx_end = trl_intervals[1:] - 1
    idx_end = idx_end - np.r_[rng.integers(step // 10, size=nTrials - 1), 0]
    shortest_trial = np.min(idx_end - idx_start)
    idx_offset = -rng.choice(np.arange(0.05 * shortest_trial, 0.2 * shortest_trial, dtype=int), size=nTrials,
                             replace=True)
    trldef = np.vstack([idx_start, idx_end, idx_offset]).T
    data = np.vstack([spike_samples, channels, units]).T
    return SpikeData(data=data, trialdefinition=trldef, dimord=["sample", "channel", "unit"], samplerate=samplerate)
