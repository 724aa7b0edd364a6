"""spy.synthdata on the device: the kernels of syncopy_amd/csrc/synth_kernel.h through the torch-free ABI at the shapes of
tests/synth_drive.py (against the oracle, and the coupled AR(2) kernel bit for bit against its CPU emulation), a tensor
of more than 2^31 elements, every front end with device=True against its host path, chunked uploads, and chains that
never touch the host."""
import types

import numpy as np
import pytest

import synth_drive as SD
import synth_oracle as O
import syncopy_amd as spy

pytestmark = pytest.mark.gpu

S = spy.synthdata


@pytest.fixture(scope="module")
def dev():
    """`dev` of synth_drive on abi.Device"""
    from syncopy_amd import abi
    d = abi.Device(0)
    yield types.SimpleNamespace(ar2=d.synth_ar2, phase=d.synth_phase, tile=d.synth_tile)
    d.close()


@pytest.fixture(scope="module")
def emu():
    return SD.emu_dev()


def resident(obj):
    """the object's data lies on the device and nobody has fetched it"""
    return obj._data is None and obj._pending is not None and obj._device is not None and obj._device.is_cuda


# ---- the kernels through the ABI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntrials", SD.TRIALS)
@pytest.mark.parametrize("nsamples", SD.SAMPLES)
@pytest.mark.parametrize("name", list(SD.COUPLED))
def test_ar2_coupled(dev, emu, name, nsamples, ntrials):
    got = SD.check_ar2_coupled(dev, name, nsamples, ntrials)
    SD.same_bits(got, SD.check_ar2_coupled(emu, name, nsamples, ntrials))


def test_ar2_table_in_global_memory(dev, emu):
    """256 channels with about 32 000 couplings: 260 KB of table do not fit the LDS of a workgroup"""
    adj = O.mk_RandomAdjMat(256, conn_thresh=0.5, seed=4)
    rowptr, col, _ = S.coupling_table(adj)
    r = SD.route_ar2(2, 19, 256, rowptr, col)
    assert r.err is None and (r.coupled, r.csr_in_lds, r.block) == (1, 0, 256) and 8 * r.nnz > 160 * 1024
    noise, seeds = SD.ar2_inputs(adj, 19, 2)
    got = dev.ar2(noise, adj, (0.55, -0.8))
    SD.within_ar2_bounds(got, SD.ar2_expected(adj, (0.55, -0.8), 19, seeds), "256 channels, table in global memory")
    SD.same_bits(got, emu.ar2(noise, adj, (0.55, -0.8)))


def test_ar2_largest_workgroup(dev, emu):
    """1024 channels, one thread each; 1025 are refused"""
    adj = O.mk_RandomAdjMat(1024, conn_thresh=0.01, seed=5)
    noise, seeds = SD.ar2_inputs(adj, 11, 1)
    got = dev.ar2(noise, adj, (0.55, -0.8))
    SD.within_ar2_bounds(got, SD.ar2_expected(adj, (0.55, -0.8), 11, seeds), "1024 channels")
    from syncopy_amd._lib import SpyHipError
    with pytest.raises(SpyHipError, match="more than 1024 channels"):
        dev.ar2(np.zeros((1, 3, 1025)), np.zeros((1025, 1025)), (0.55, -0.8))


@pytest.mark.parametrize("ntrials", SD.TRIALS)
@pytest.mark.parametrize("nsamples", SD.SAMPLES)
@pytest.mark.parametrize("name", list(SD.UNCOUPLED))
def test_ar2_uncoupled(dev, name, nsamples, ntrials):
    SD.check_ar2_uncoupled(dev, name, nsamples, ntrials)


@pytest.mark.parametrize("return_phase", (True, False))
@pytest.mark.parametrize("rand_ini", (True, False))
@pytest.mark.parametrize("nchan", SD.PHASE_CHANNELS)
@pytest.mark.parametrize("nsamples", SD.PHASE_SAMPLES)
def test_phase(dev, nsamples, nchan, rand_ini, return_phase):
    SD.check_phase(dev, nsamples, nchan, rand_ini, return_phase)


def test_phase_several_workgroups_and_a_second(dev):
    SD.check_phase(dev, 9, 130, True, True, ntrials=3)
    SD.check_phase(dev, 1000, 3, True, False, ntrials=2)          # phases up to 2 pi 60: the cosine's range reduction


@pytest.mark.parametrize("ntrials", SD.TRIALS)
@pytest.mark.parametrize("nchan", SD.TILE_CHANNELS)
@pytest.mark.parametrize("nsamples", SD.TILE_SAMPLES)
def test_tile(dev, nsamples, nchan, ntrials):
    SD.check_tile(dev, nsamples, nchan, ntrials)


def test_tile_past_2_31_elements():
    """2057 trials x 4096 samples x 255 channels = 2.15e9 element lanes (8.6 GB), compared on the device"""
    import torch
    from syncopy_amd import backend
    T, n, c = 2057, 4096, 255
    assert T * n * c > 2 ** 31
    col = torch.from_numpy(O.harmonic(30, 1000, nSamples=n, nChannels=1)[:, 0].copy()).cuda()
    out = torch.empty((T * n, c), dtype=torch.float32, device="cuda")
    backend.synth_tile(col, T, out)
    view = out.view(T, n, c)
    assert bool((view[-1] == col[:, None]).all()) and bool((view[0] == col[:, None]).all())
    assert bool((view == col.view(1, n, 1)).all())


def test_phase_past_2_31_elements(emu):
    """the last trials of 2057 x 4096 x 255 values of noise drawn on the device, against the emulated kernel"""
    import torch
    from syncopy_amd import backend
    T, n, c = 2057, 4096, 255
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    wn = torch.randn((T, n, c), generator=g, device="cuda", dtype=torch.float32)
    _, lin, _, rel_eps = SD.phase_inputs(60, 0.1, 1000, c, n, False, [0])
    ps0 = torch.rand((T, c), generator=g, device="cuda", dtype=torch.float32)
    out = torch.empty((T * n, c), dtype=torch.float32, device="cuda")
    backend.synth_phase(wn, torch.from_numpy(lin).cuda(), ps0, rel_eps, False, out)
    got = out.view(T, n, c)[-1:].cpu().numpy()
    SD.same_bits(got, emu.phase(wn[-1:].cpu().numpy(), lin, ps0[-1:].cpu().numpy(), rel_eps, False))


# ---- the front ends ----------------------------------------------------------------------------------------------------------
ADJ = O.mk_RandomAdjMat(6, seed=8)
BITWISE = {
    "white_noise": lambda **kw: S.white_noise(nSamples=70, nChannels=5, **kw),
    "linear_trend": lambda **kw: S.linear_trend(3.5, nSamples=70, nChannels=4, **kw),
    "harmonic": lambda **kw: S.harmonic(30, samplerate=500, nSamples=70, nChannels=3, **kw),
    "phase": lambda **kw: S.phase_diffusion(60, nSamples=70, nChannels=5, return_phase=True, **kw),
    "phase rand_ini": lambda **kw: S.phase_diffusion(60, eps=0.3, nSamples=70, nChannels=5, rand_ini=True, return_phase=True, **kw),
    "red_noise": lambda **kw: S.red_noise(0.9, nSamples=70, nChannels=5, **kw),
    "ar2_network uncoupled": lambda **kw: S.ar2_network(AdjMat=np.zeros((4, 4)), nSamples=70, **kw),
}


def _same_object(got, want):
    assert isinstance(got, spy.AnalogData) and resident(got)
    assert got.samplerate == want.samplerate and np.array_equal(got.trialdefinition, want.trialdefinition)
    assert list(got.channel) == list(want.channel) and tuple(got.data_shape) == want.data.shape
    assert got.data_dtype == np.float32


@pytest.mark.parametrize("seed_per_trial", (True, False))
@pytest.mark.parametrize("name", list(BITWISE))
def test_front_end_gives_the_hosts_bits(name, seed_per_trial):
    kw = dict(nTrials=3, seed=21, seed_per_trial=seed_per_trial)
    got, want = BITWISE[name](device=True, **kw), BITWISE[name](**kw)
    _same_object(got, want)
    SD.same_bits(got.data, want.data)


def test_front_end_coupled_ar2():
    for adj in (None, ADJ):
        kw = dict(AdjMat=adj, nSamples=200, nTrials=3, seed=4, samplerate=200)
        got, want = S.ar2_network(device=True, **kw), S.ar2_network(**kw)
        _same_object(got, want)
        SD.within_ar2_bounds(got.data.reshape(3, 200, -1), want.data.reshape(3, 200, -1), "front end")


def test_front_end_cosine():
    for rand_ini in (False, True):
        kw = dict(nSamples=300, nChannels=3, rand_ini=rand_ini, nTrials=2, seed=9)
        got, want = S.phase_diffusion(60, device=True, **kw), S.phase_diffusion(60, **kw)
        _same_object(got, want)
        worst = float(np.max(np.abs(got.data.astype(np.float64) - want.data.astype(np.float64)))) / SD.EPS32
        print(f"cos, rand_ini={rand_ini}: largest |d| = {worst:.3g} eps32")
        assert worst <= 4.0


def test_front_end_refuses():
    with pytest.raises(ValueError, match="nTrials"):
        S.white_noise(nTrials=None, device=True)
    with pytest.raises(ValueError, match="1024"):
        S.red_noise(0.9, nSamples=3, nChannels=1025, nTrials=1, device=True)
    with pytest.raises(ValueError, match="2 samples"):
        S.red_noise(0.9, nSamples=1, nTrials=1, device=True)


CHUNKED = {
    "white_noise": (4, lambda: S.white_noise(nSamples=33, nChannels=5, nTrials=5, seed=2, device=True)),
    "phase_diffusion": (4, lambda: S.phase_diffusion(60, nSamples=33, nChannels=5, rand_ini=True, nTrials=5, seed=2, device=True)),
    "ar2_network": (8, lambda: S.ar2_network(AdjMat=O.mk_RandomAdjMat(5, seed=1), nSamples=33, nTrials=5, seed=2, device=True)),
    "red_noise": (8, lambda: S.red_noise(0.9, nSamples=33, nChannels=5, nTrials=5, seed=2, device=True)),
}


@pytest.mark.parametrize("name", list(CHUNKED))
def test_chunked_upload(name, monkeypatch):
    """5 trials travel in 3 chunks of 2, 2 and 1: the same bits as in one"""
    itemsize, make = CHUNKED[name]
    whole = make().data
    calls = []
    draw = S.draw_noise
    monkeypatch.setattr(S, "draw_noise", lambda seeds, *a: calls.append(len(seeds)) or draw(seeds, *a))
    monkeypatch.setattr(S, "CHUNK_BYTES", 2 * 33 * 5 * itemsize + 1)
    parts = make().data
    assert calls == [2, 2, 1]
    SD.same_bits(parts, whole)


# ---- chains that stay on the device ---------------------------------------------------------------------------------------
def test_harmonic_plus_noise_into_freqanalysis():
    """the tutorial's first line: resident through the operators, and read by freqanalysis where it lies (what that front
    end does with its input beyond device_data() is its own)"""
    kw = dict(nSamples=1000, nChannels=3, nTrials=10)
    harm, noise = S.harmonic(freq=30, samplerate=1000, device=True, **kw), S.white_noise(seed=1, device=True, **kw)
    data = 2 * harm + noise
    assert resident(harm) and resident(noise) and data._data is None
    spec = spy.freqanalysis(data, method="mtmfft", keeptrials=False)
    assert harm._data is None and noise._data is None
    power = np.asarray(spec.data).reshape(len(spec.freq), -1)
    assert np.all(spec.freq[np.argmax(power, axis=0)] == 30)
    want = 2 * S.harmonic(freq=30, samplerate=1000, **kw).data + S.white_noise(seed=1, **kw).data
    SD.same_bits(data.data, want)


PEAK_SMOOTH = 21        # bins of 1 Hz in the running mean over the averaged spectrum
PEAK_BOUND = 5.0        # Hz


def _peak_bins(data):
    """per channel the frequency of the largest 1 Hz bin of the trial-averaged spectrum, raw and after a running mean
    over PEAK_SMOOTH bins"""
    spec = spy.freqanalysis(data, method="mtmfft", keeptrials=False)
    freq = np.asarray(spec.freq)
    power = np.asarray(spec.data).reshape(len(freq), -1).astype(np.float64)
    assert np.allclose(np.diff(freq), 1.0)
    half = PEAK_SMOOTH // 2
    kernel = np.ones(PEAK_SMOOTH) / PEAK_SMOOTH
    smooth = np.stack([np.convolve(power[:, c], kernel, mode="valid") for c in range(power.shape[1])], axis=1)
    return freq[np.argmax(power, axis=0)], freq[half + np.argmax(smooth, axis=0)]


def test_default_ar2_network_peaks_at_its_frequency():
    """50 trials x 1000 samples of the default 2 -> 1 system against ar2_peak_freq(0.55, -0.8, 1000) = 199.94 Hz, on the
    1 Hz bins of the averaged spectrum.

    The peak of this process is about 35 Hz wide, and a 1 Hz bin of 50 averaged periodograms scatters by 14 %, so the
    largest RAW bin is not within one bin of the peak for the reference itself: over the seeds 1 .. 20 the host path
    (Hann taper, both channels) has it between 195 and 205 Hz, standard deviation 2.3 Hz.  A running mean over 21 bins
    brings the host path to 196 .. 203 Hz, standard deviation 1.6 Hz, largest distance 3.9 Hz.  The bound is three of
    those standard deviations, 5 Hz, set from the host path before the device route was run.  What the device route
    has to add to that is nothing: its largest bins, raw and smoothed, are the host path's for the same seed."""
    kw = dict(nTrials=50, nSamples=1000, seed=3)
    data = S.ar2_network(device=True, **kw)
    assert resident(data) and tuple(data.data_shape) == (50_000, 2)
    peak = float(S.ar2_peak_freq(0.55, -0.8, data.samplerate))
    raw, smooth = _peak_bins(data)
    host_raw, host_smooth = _peak_bins(S.ar2_network(**kw))
    print(f"peak {peak:.2f} Hz; device: raw {raw}, smoothed {smooth}; host path: raw {host_raw}, smoothed {host_smooth}")
    assert abs(peak - 199.94) < 0.01
    assert np.all(np.abs(smooth - peak) <= PEAK_BOUND)
    assert np.array_equal(raw, host_raw) and np.array_equal(smooth, host_smooth)
