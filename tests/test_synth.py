"""spy.synthdata (syncopy_amd/synthdata.py, csrc/synth.hip) without a GPU: the host generators against the NumPy model of
the reference (tests/synth_oracle.py), bit for bit; the route through its shim with every refusal; and the library's own
launchers and kernels at their dispatch edges through the CPU emulation (tests/emu/synth_emu.cpp)."""
import numpy as np
import pytest

import synth_drive as SD
import synth_oracle as O
import syncopy_amd as spy

S = spy.synthdata


def same(a, b):
    assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# name -> (generator, oracle, positional arguments, keywords of the trial function)
ADJ = O.mk_RandomAdjMat(4, seed=3)
GENERATORS = {
    "white_noise": (S.white_noise, O.white_noise, (), dict(nSamples=40, nChannels=3)),
    "linear_trend": (S.linear_trend, O.linear_trend, (2.5,), dict(nSamples=33, nChannels=3)),
    "harmonic": (S.harmonic, O.harmonic, (30,), dict(nSamples=50, nChannels=2)),
    "phase_diffusion": (S.phase_diffusion, O.phase_diffusion, (60,), dict(nSamples=70, nChannels=3)),
    "phase_diffusion rand_ini": (S.phase_diffusion, O.phase_diffusion, (60,), dict(nSamples=70, nChannels=3, rand_ini=True)),
    "phase_diffusion phase": (S.phase_diffusion, O.phase_diffusion, (60,), dict(nSamples=70, nChannels=3, return_phase=True)),
    "phase_diffusion rand_ini phase": (S.phase_diffusion, O.phase_diffusion, (60,),
                                       dict(nSamples=70, nChannels=3, eps=0.3, rand_ini=True, return_phase=True)),
    "ar2_network default": (S.ar2_network, O.ar2_network, (), dict(nSamples=60)),
    "ar2_network coupled": (S.ar2_network, O.ar2_network, (), dict(AdjMat=ADJ, nSamples=60, alphas=(0.5, -0.7))),
    "red_noise": (S.red_noise, O.red_noise, (0.9,), dict(nSamples=60, nChannels=3)),
}
SEEDED = [k for k in GENERATORS if not k.startswith(("linear", "harmonic"))]


@pytest.mark.parametrize("name", list(GENERATORS))
def test_single_trial(name):
    gen, oracle, args, kw = GENERATORS[name]
    kw = dict(kw, seed=7) if name in SEEDED else kw
    same(gen(*args, nTrials=None, **kw), O.collect(oracle, *args, nTrials=None, **kw))


@pytest.mark.parametrize("seed_per_trial", (True, False))
@pytest.mark.parametrize("ntrials", (1, 3))
@pytest.mark.parametrize("name", list(GENERATORS))
def test_trials(name, ntrials, seed_per_trial):
    gen, oracle, args, kw = GENERATORS[name]
    out = gen(*args, nTrials=ntrials, seed=12, seed_per_trial=seed_per_trial, samplerate=500, **kw)
    want = O.collect(oracle, *args, nTrials=ntrials, seed=12, seed_per_trial=seed_per_trial, samplerate=500, **kw)
    assert isinstance(out, spy.AnalogData) and out.samplerate == 500
    same(out.data, np.concatenate(want))
    assert np.array_equal(out.trialdefinition, O.trialdefinition(ntrials, want[0].shape[0], 500))
    for got, trial in zip(out.trials, want):
        same(np.ascontiguousarray(got), trial)
    if name in SEEDED and ntrials > 1:
        assert np.array_equal(want[0], want[1]) == (not seed_per_trial)


@pytest.mark.parametrize("name", list(GENERATORS))
def test_without_a_seed(name):
    """seed=None: shapes and dtypes only; the trials of a random generator differ"""
    gen, oracle, args, kw = GENERATORS[name]
    want = O.collect(oracle, *args, nTrials=None, seed=1, **kw)
    one = gen(*args, nTrials=None, **kw)
    assert one.shape == want.shape and one.dtype == want.dtype
    out = gen(*args, nTrials=2, **kw)
    assert out.data.shape == (2 * want.shape[0], want.shape[1]) and out.data.dtype == want.dtype
    if name in SEEDED:
        assert not np.array_equal(out.trials[0], out.trials[1])


def test_samplerate_reaches_the_trial_function():
    """harmonic and phase_diffusion have the parameter: the collector forwards it (utils.py:57-59)"""
    for rate in (200, 1000):
        same(S.harmonic(30, samplerate=rate, nTrials=2, nSamples=40).data,
             np.concatenate(O.collect(O.harmonic, 30, nTrials=2, samplerate=rate, nSamples=40)))
        same(S.phase_diffusion(30, samplerate=rate, nTrials=2, nSamples=40, seed=3).data,
             np.concatenate(O.collect(O.phase_diffusion, 30, nTrials=2, samplerate=rate, nSamples=40, seed=3)))
    assert not np.array_equal(S.harmonic(30, samplerate=200, nTrials=None), S.harmonic(30, samplerate=1000, nTrials=None))
    assert S.harmonic(30, nTrials=1).trialdefinition.tolist() == [[0, 1000, -1000]]


def test_defaults_are_the_references():
    """100 trials of 1000 samples on 2 channels at 1000 Hz"""
    out = S.white_noise(seed=1)
    assert out.data.shape == (100_000, 2) and out.samplerate == 1000 and len(out.trials) == 100
    same(out.data, np.concatenate(O.collect(O.white_noise, seed=1)))


def test_phase_diffusion_is_float32_throughout():
    for flags in (dict(), dict(rand_ini=True), dict(return_phase=True)):
        assert S.phase_diffusion(60, nTrials=None, seed=1, **flags).dtype == np.float32
    assert S.phase_diffusion(np.float64(60), nTrials=None, seed=1).dtype == np.float32      # (float64 under NumPy 2's rules)


def test_existing_generators_are_unchanged():
    """white_noise and ar2_network with the arguments they had before seed_per_trial and device were added: still the
    reference's stream for the seed (what the golden files and the benchmark input are pinned to)"""
    a = S.ar2_network(AdjMat=np.zeros((3, 3)), nSamples=50, nTrials=2, seed=42).data
    b = np.concatenate(O.collect(O.ar2_network, AdjMat=np.zeros((3, 3)), nSamples=50, nTrials=2, seed=42))
    same(a, b)
    same(S.white_noise(nSamples=20, nChannels=2, seed=3, nTrials=2).data,
         np.concatenate([np.random.default_rng(s).normal(size=(20, 2)).astype("f4")
                         for s in np.random.default_rng(3).integers(1_000_000, size=2)]))


def test_lag2_parameter_is_float32_whatever_its_type():
    """NumPy 1 casts any scalar that multiplies the float32 signal to float32 (analog.py:249); a float64 scalar under
    NumPy 2 would not be"""
    kw = dict(AdjMat=ADJ, nSamples=40, nTrials=None, seed=2)
    want = O.ar2_network(AdjMat=ADJ, nSamples=40, alphas=(0.5, -0.7), seed=2)
    same(S.ar2_network(alphas=(0.5, -0.7), **kw), want)
    same(S.ar2_network(alphas=(np.float64(0.5), np.float64(-0.7)), **kw), want)
    same(S.ar2_network(alphas=np.array([0.5, -0.7]), **kw), want)


def test_nTrials_is_checked():
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            S.harmonic(30, nTrials=bad)
    with pytest.raises(ValueError):
        S.harmonic(30, nTrials=None, device=True)           # device=True returns an object


def test_cfg_carries_the_keywords():
    """utils.py:48: collect_trials sits behind unwrap_cfg"""
    cfg = dict(nTrials=2, nSamples=30, nChannels=3, seed=4)
    want = np.concatenate(O.collect(O.white_noise, **cfg))
    same(S.white_noise(cfg).data, want)
    same(S.white_noise(cfg=cfg).data, want)
    same(S.white_noise(dict(cfg, nTrials=None, seed=6)), O.white_noise(30, 3, 6))
    same(S.harmonic(30, cfg=dict(nTrials=None, nSamples=20)), O.harmonic(30, 1000, nSamples=20))
    assert cfg == dict(nTrials=2, nSamples=30, nChannels=3, seed=4)          # the caller's dictionary is left alone
    with pytest.raises(Exception, match="nSamples"):
        S.white_noise(cfg, nSamples=10)                                       # set in both


def test_mk_RandomAdjMat():
    for kw in (dict(), dict(nChannels=8, seed=3), dict(nChannels=20, conn_thresh=0.5, max_coupling=0.4, seed=1), dict(nChannels=5, conn_thresh=1.0, seed=2)):
        a, b = S.mk_RandomAdjMat(**dict(kw, seed=kw.get("seed", 9))), O.mk_RandomAdjMat(**dict(kw, seed=kw.get("seed", 9)))
        assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b)
        assert np.all(np.diag(a) == 0)
        sums = a.sum(axis=0)
        assert np.all((sums == 0) | np.isclose(sums, kw.get("max_coupling", 0.25)))
    assert S.mk_RandomAdjMat().shape == (3, 3)


def test_ar2_peak_freq():
    for args in ((0.55, -0.8), (0.55, -0.8, 200), (1.0, -0.9, 1000), (np.array([0.5, 0.2]), np.array([-0.8, -0.5]), 100)):
        assert np.array_equal(S.ar2_peak_freq(*args), O.ar2_peak_freq(*args))
    assert abs(S.ar2_peak_freq(0.55, -0.8, 200) - 40) < 0.02           # the Dhamala system: 40 Hz at 200 Hz
    for args in ((2.0, -0.5), (0.5, 0.1), (np.array([0.5, 2.0]), np.array([-0.8, -0.5]))):
        with pytest.raises(ValueError, match="No complex roots"):
            S.ar2_peak_freq(*args)


def test_coupling_table():
    adj = np.array([[0.5, 0.25, 0], [0, 0, 0], [0.125, 0, -0.0]])
    rowptr, col, w = S.coupling_table(adj)                    # rows of adj.T: the senders of each receiver
    assert rowptr.tolist() == [0, 2, 3, 3] and col.tolist() == [0, 2, 0] and w.tolist() == [0.5, 0.125, 0.25]
    assert (rowptr.dtype, col.dtype, w.dtype) == (np.int32, np.int32, np.float32)
    rowptr, col, w = S.coupling_table(np.zeros((4, 4)))
    assert rowptr.tolist() == [0] * 5 and col.size == 0 and w.size == 0


def test_noise_in_one_call_is_the_row_by_row_stream():
    """what the device route uploads: one draw of (nSamples, nChannels) is the reference's two initial rows and then one
    row per sample (analog.py:245-250)"""
    rng = np.random.default_rng(77)
    rows = [rng.normal(size=(2, 3))] + [rng.normal(size=3)[None] for _ in range(2, 9)]
    assert np.array_equal(np.concatenate(rows), np.random.default_rng(77).normal(size=(9, 3)))
    noise = S.draw_noise([5, 6, 7, 8, 9], 9, 3, np.float64)
    assert np.array_equal(noise, np.stack([np.random.default_rng(s).normal(size=(9, 3)) for s in (5, 6, 7, 8, 9)]))
    same(S.draw_noise([5, 6], 9, 3, np.float32), np.stack([O.white_noise(9, 3, s) for s in (5, 6)]))
    assert S.DRAW_THREADS <= 16


def test_trial_chunks():
    assert S._trial_chunks(5, 100, 250) == [(0, 2), (2, 4), (4, 5)]
    assert S._trial_chunks(5, 100, 50) == [(k, k + 1) for k in range(5)]         # at least one trial each
    assert S._trial_chunks(5, 100, 1 << 30) == [(0, 5)]
    assert S.CHUNK_BYTES == 512 << 20


# ---- the route -----------------------------------------------------------------------------------------------------------------
def test_route_ar2():
    rowptr, col, _ = S.coupling_table(O.mk_RandomAdjMat(65, seed=1))
    r = SD.route_ar2(3, 67, 65, rowptr, col)
    nnz = int(rowptr[-1])
    assert r.err is None and (r.coupled, r.csr_in_lds, r.block, r.grid, r.nnz) == (1, 1, 128, 3, nnz)
    assert r.lds_bytes == 2 * 4 * 65 + 4 * 66 + 8 * nnz
    r = SD.route_ar2(3, 67, 65, rowptr, col, lds_per_block=2 * 4 * 65 + 4 * 66 + 8 * nnz - 1)     # one byte short: global
    assert (r.coupled, r.csr_in_lds, r.lds_bytes, r.block, r.grid) == (1, 0, 2 * 4 * 65, 128, 3)
    for nchan, block in ((2, 64), (64, 64), (65, 128), (1024, 1024)):     # the last channel sends to the first
        rp = np.zeros(nchan + 1, dtype=np.int32)
        rp[1:] = 1
        r = SD.route_ar2(2, 5, nchan, rp, [nchan - 1])
        assert r.err is None and (r.coupled, r.block, r.grid) == (1, block, 2), (nchan, r)
    # no entry off the diagonal: one thread per series
    for rowptr, col in (([0, 0, 0, 0], []), ([0, 1, 1, 2], [0, 2])):
        r = SD.route_ar2(100, 9, 3, rowptr, col)
        assert r.err is None and (r.coupled, r.csr_in_lds, r.block, r.grid, r.lds_bytes) == (0, 0, 256, 2, 0)
    assert SD.route_ar2(0, 9, 3, [0, 0, 0, 0], []).err is None
    assert SD.shim().sr_max_channels() == 1024 == S.MAX_DEVICE_CHANNELS


def test_route_ar2_refuses():
    ok = dict(ntrials=2, nsamples=5, nchan=3, rowptr=[0, 1, 1, 3], col=[1, 0, 2])
    assert SD.route_ar2(**ok).err is None
    big = np.zeros(1026, dtype=np.int32)
    assert SD.route_ar2(1, 5, 1025, big, []).err == "more than 1024 channels"
    assert SD.route_ar2(1, 5, 1024, big[:1025], []).err is None
    assert SD.route_ar2(**{**ok, "nsamples": 1}).err == "a trial has fewer than 2 samples"
    assert SD.route_ar2(**{**ok, "ntrials": -1}).err == "negative trial count"
    assert SD.route_ar2(**{**ok, "nchan": 0}).err == "no channels"
    assert SD.route_ar2(**{**ok, "nsamples": 1 << 60}).err == "the tensor is too large"
    assert SD.route_ar2(**{**ok, "ntrials": 1 << 40, "nsamples": 1 << 20}).err == "the tensor is too large"
    assert SD.route_ar2(**{**ok, "rowptr": [1, 1, 1, 3]}).err == "the coupling table does not begin at 0"
    malformed = "a row of the coupling table is malformed"
    assert SD.route_ar2(**{**ok, "rowptr": [0, 2, 1, 3]}).err == malformed
    assert SD.route_ar2(**{**ok, "rowptr": [0, 4, 4, 4], "col": [0, 1, 2, 2]}).err == malformed       # more senders than channels
    assert SD.route_ar2(**{**ok, "col": [3, 0, 2]}).err == "a sender lies outside the channels"
    assert SD.route_ar2(**{**ok, "col": [-1, 0, 2]}).err == "a sender lies outside the channels"
    assert SD.route_ar2(**{**ok, "col": [1, 2, 0]}).err == "the senders of a receiver are not ascending"
    assert SD.route_ar2(**{**ok, "col": [1, 2, 2]}).err == "the senders of a receiver are not ascending"


def test_route_phase_and_tile():
    r = SD.route_phase(3, 65, 65)
    assert r.err is None and (r.block, r.grid) == (256, 1)
    assert SD.route_phase(1000, 1, 256).grid == 1000 and SD.route_phase(1, 1, 257).grid == 2
    assert SD.route_phase(1, 0, 2).err == "a trial has no samples" and SD.route_phase(1, 1, 0).err == "no channels"
    assert SD.route_phase(1 << 31, 1, 256).err == "too many series"
    assert SD.route_phase(1, 1, 2000).err is None                      # the channel cap is the AR(2) workgroup's alone
    r = SD.route_tile(3, 130, 68)
    assert r.err is None and (r.lane_bytes, r.lanes, r.grid) == (16, 3 * 130 * 17, (3 * 130 * 17 + 255) // 256)
    assert SD.route_tile(3, 130, 65).lane_bytes == 4 and SD.route_tile(3, 130, 65).lanes == 3 * 130 * 65
    assert SD.route_tile(3, 130, 68, out_addr=(1 << 40) + 8).lane_bytes == 4          # the output off a 16-byte boundary
    assert SD.route_tile(3, 130, 68, out_addr=(1 << 40) + 2).err == "the output is not aligned to its element type"
    assert SD.route_tile(1000, 4096, 256, max_blocks=4096).grid == 4096
    assert SD.route_tile(0, 5, 4).lanes == 0 and SD.route_tile(1, 0, 4).err == "a trial has no samples"


# ---- the kernels through the library's launchers, emulated -----------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    return SD.emu_dev()


@pytest.mark.parametrize("ntrials", SD.TRIALS)
@pytest.mark.parametrize("nsamples", SD.SAMPLES)
@pytest.mark.parametrize("name", list(SD.COUPLED))
def test_emu_ar2_coupled(dev, name, nsamples, ntrials):
    import build_emu
    build_emu.launches(SD.emu())
    SD.check_ar2_coupled(dev, name, nsamples, ntrials)
    adj = SD.COUPLED[name][0]
    nchan = 2 if adj is None else adj.shape[0]
    log = build_emu.launches(SD.emu())
    assert log.shape[0] == 1 and log[0, :4].tolist() == [ntrials, 1, 1, (nchan + 63) // 64 * 64] and log[0, 6] > 8 * nchan


@pytest.mark.parametrize("name", list(SD.COUPLED))
def test_emu_ar2_table_in_global_memory(dev, name):
    """the LDS budget shrunk to the state vectors: the table is read from global memory and the bits are the same"""
    import build_emu
    lib = SD.emu()
    adj = SD.COUPLED[name][0]
    nchan = 2 if adj is None else adj.shape[0]
    small = build_emu.ctx(lib)
    lib.emu_ctx_set_chip(small, 0, 8 * nchan)
    try:
        build_emu.launches(lib)
        got = SD.check_ar2_coupled(SD.emu_dev(small), name, 67, 3)
        assert build_emu.launches(lib)[0].tolist() == [3, 1, 1, (nchan + 63) // 64 * 64, 1, 1, 8 * nchan]
        SD.same_bits(got, SD.check_ar2_coupled(dev, name, 67, 3))
    finally:
        lib.emu_ctx_destroy(small)


@pytest.mark.parametrize("ntrials", SD.TRIALS)
@pytest.mark.parametrize("nsamples", SD.SAMPLES)
@pytest.mark.parametrize("name", list(SD.UNCOUPLED))
def test_emu_ar2_uncoupled(dev, name, nsamples, ntrials):
    import build_emu
    build_emu.launches(SD.emu())
    SD.check_ar2_uncoupled(dev, name, nsamples, ntrials)
    nchan = SD.UNCOUPLED[name][0].shape[0]
    assert build_emu.launches(SD.emu()).tolist() == [[(ntrials * nchan + 255) // 256, 1, 1, 256, 1, 1, 0]]


def test_emu_the_routes_agree(dev):
    """a table whose only entries are on the diagonal takes the series kernel; the same system with a coupling of 0.0f
    spelled out as an entry off the diagonal takes the workgroup kernel: the same bits"""
    noise, _ = SD.ar2_inputs(np.zeros((3, 3)), 67, 3)
    rc, a = SD.emu_ar2_raw(noise, [0, 1, 1, 2], [0, 2], [0.1, -0.2], (0.5, -0.3))
    assert rc == 0
    rc, b = SD.emu_ar2_raw(noise, [0, 2, 2, 3], [0, 1, 2], [0.1, 0.0, -0.2], (0.5, -0.3))
    assert rc == 0
    SD.same_bits(a, b)


def test_emu_ar2_refuses(dev):
    noise = np.zeros((1, 5, 3))
    assert SD.emu_ar2_raw(noise, [0, 1, 1, 3], [1, 2, 0], [1, 1, 1], (0.5, -0.3))[0] == -1
    assert SD.emu_ar2_raw(np.zeros((1, 1, 3)), [0, 0, 0, 0], [], [], (0.5, -0.3))[0] == -1
    rc, out = SD.emu_ar2_raw(np.zeros((0, 5, 3)), [0, 0, 0, 0], [], [], (0.5, -0.3))
    assert rc == 0 and out.size == 0


@pytest.mark.parametrize("return_phase", (True, False))
@pytest.mark.parametrize("rand_ini", (True, False))
@pytest.mark.parametrize("nchan", SD.PHASE_CHANNELS)
@pytest.mark.parametrize("nsamples", SD.PHASE_SAMPLES)
def test_emu_phase(dev, nsamples, nchan, rand_ini, return_phase):
    SD.check_phase(dev, nsamples, nchan, rand_ini, return_phase)


def test_emu_phase_two_workgroups(dev):
    SD.check_phase(dev, 9, 130, True, True, ntrials=3)           # 390 series


@pytest.mark.parametrize("ntrials", SD.TRIALS)
@pytest.mark.parametrize("nchan", SD.TILE_CHANNELS)
@pytest.mark.parametrize("nsamples", SD.TILE_SAMPLES)
def test_emu_tile(dev, nsamples, nchan, ntrials):
    SD.check_tile(dev, nsamples, nchan, ntrials)


def test_emu_tile_grid_stride():
    """two workgroups walk 3 x 130 x 17 lanes in several rounds"""
    import build_emu
    lib = SD.emu()
    build_emu.launches(lib)
    SD.check_tile(SD.emu_dev(lib.few), 130, 68, 3)
    assert build_emu.launches(lib)[:, :4].tolist() == [[2, 1, 1, 256]] * 2
