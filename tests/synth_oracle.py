"""NumPy model of the reference's synthetic-data generators for tests/test_synth.py and tests/test_gpu_synth.py: a plain
restatement of the per-trial functions of syncopy/synthdata/analog.py and of the trial loop of
syncopy/synthdata/utils.py: collect_trials, with the casts that NumPy 1 (value-based casting, under which the reference
was written) applies written out, so that the model gives the same bits under NumPy 2.  Nothing here imports the package
under test."""
import inspect

import numpy as np

TWO_PI = np.pi * 2


def white_noise(nSamples=1000, nChannels=2, seed=None):
    """analog.py:38-40"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(nSamples, nChannels)).astype("f4")


def linear_trend(y_max, nSamples=1000, nChannels=2):
    """analog.py:62-63"""
    trend = np.linspace(0, y_max, nSamples, dtype="f4")
    return np.column_stack([trend for _ in range(nChannels)])


def harmonic(freq, samplerate, nSamples=1000, nChannels=2):
    """analog.py:88-91"""
    tvec = np.arange(nSamples) * 1 / samplerate
    harm = np.cos(2 * np.pi * freq * tvec, dtype="f4")
    return np.column_stack([harm for _ in range(nChannels)])


def phase_diffusion(freq, eps=0.1, samplerate=1000, nChannels=2, nSamples=1000, rand_ini=False, return_phase=False,
                    seed=None):
    """analog.py:161-182.  NumPy 1: a Python float or a float64 SCALAR that meets a float32 array is cast to float32, and
    the result is float32 (lines 165, 170, 175); every array below is therefore float32."""
    wn = white_noise(nSamples=nSamples, nChannels=nChannels, seed=seed)                 # :161
    tvec = np.linspace(0, nSamples / samplerate, nSamples, dtype="f4")                  # :163
    omega0 = 2 * np.pi * freq                                                           # :164
    lin_phase = np.tile(np.float32(omega0) * tvec, (nChannels, 1)).T                    # :165
    if rand_ini:                                                                        # :168-171
        rng = np.random.default_rng(seed)
        ps0 = np.float32(2 * np.pi) * rng.uniform(size=nChannels).astype("f4")
        lin_phase += ps0
    rel_eps = np.sqrt(omega0 / samplerate * eps)                                        # :174, a float64 scalar
    brown_incr = np.float32(rel_eps) * wn                                               # :175
    assert brown_incr.dtype == np.float32 and lin_phase.dtype == np.float32
    phases = lin_phase + np.cumsum(brown_incr, axis=0)                                  # :178
    assert phases.dtype == np.float32
    return phases if return_phase else np.cos(phases)                                  # :179-182


def ar2_network(AdjMat=None, nSamples=1000, alphas=(0.55, -0.8), seed=None):
    """analog.py:231-252"""
    if AdjMat is None:
        AdjMat = np.zeros((2, 2), dtype=np.float32)
        AdjMat[1, 0] = 0.25
    else:
        AdjMat = np.asarray(AdjMat).astype(np.float32)
    nChannels = AdjMat.shape[0]
    alpha1, alpha2 = alphas
    DiagMat = np.diag(nChannels * [alpha1])
    signal = np.zeros((nSamples, nChannels), dtype=np.float32)
    rng = np.random.default_rng(seed)
    signal[:2, :] = rng.normal(size=(2, nChannels))
    for i in range(2, nSamples):
        signal[i, :] = (DiagMat + AdjMat.T) @ signal[i - 1, :] + alpha2 * signal[i - 2, :]
        signal[i, :] += rng.normal(size=(nChannels))
    return signal


def red_noise(alpha, nSamples=1000, nChannels=2, seed=None):
    """analog.py:281-286"""
    return ar2_network(AdjMat=np.diag(np.zeros(nChannels)), nSamples=nSamples, alphas=[alpha, 0], seed=seed)


def ar2_peak_freq(a1, a2, samplerate=1):
    """analog.py:293-296"""
    if np.any((a1**2 + 4 * a2) > 0):
        raise ValueError("No complex roots!")
    return np.arccos(a1 * (a2 - 1) / (4 * a2)) * 1 / TWO_PI * samplerate


def mk_RandomAdjMat(nChannels=3, conn_thresh=0.25, max_coupling=0.25, seed=None):
    """analog.py:329-344"""
    rng = np.random.default_rng(seed)
    AdjMat = rng.random((nChannels, nChannels))
    AdjMat = (AdjMat < conn_thresh).astype(float)
    np.fill_diagonal(AdjMat, 0)
    norm = AdjMat.sum(axis=0)
    norm[norm == 0] = 1
    return AdjMat / norm[None, :] * max_coupling


def trial_seeds(nTrials, seed, seed_per_trial=True):
    """utils.py:51-55, 75-79: the seed every trial's function gets"""
    if seed is not None and seed_per_trial:
        return list(np.random.default_rng(seed).integers(1_000_000, size=nTrials))
    return [seed] * nTrials


def collect(trial_func, *args, nTrials=100, samplerate=1000, seed=None, seed_per_trial=True, **kwargs):
    """utils.py:50-86: the trials one after the other (a list), or with nTrials=None the one trial"""
    params = inspect.signature(trial_func).parameters
    if "samplerate" in params:
        kwargs["samplerate"] = samplerate
    if nTrials is None:
        if "seed" in params:
            kwargs["seed"] = seed
        return trial_func(*args, **kwargs)
    trials = []
    for s in trial_seeds(nTrials, seed, seed_per_trial):
        if "seed" in params:
            kwargs["seed"] = s
        trials.append(trial_func(*args, **kwargs))
    return trials


def trialdefinition(nTrials, nSamples, samplerate):
    """the generator-built AnalogData: trials stacked, every trigger offset -1 s"""
    starts = np.arange(nTrials) * nSamples
    return np.stack([starts, starts + nSamples, np.full(nTrials, -samplerate)], axis=1).astype(float)
