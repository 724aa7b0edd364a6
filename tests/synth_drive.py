"""What the CPU emulation (tests/test_synth.py) and the GPU tests (tests/test_gpu_synth.py) of the synthetic-data kernels
share: the emulator's driver, the route shim, and the kernel cases at the smallest shapes that can go wrong with what each
must give.  The checks are written against an object `dev` with three functions that either side supplies:
    dev.ar2(noise (T, n, c) float64, AdjMat, alphas)            -> (T, n, c) float32
    dev.phase(wn (T, n, c) float32, lin (n), ps0 (T, c), rel_eps, want_cos) -> (T, n, c) float32
    dev.tile(col (n) float32, ntrials, nchan)                    -> (T, n, c) float32
The expected values are the oracle's (tests/synth_oracle.py), trial by trial, from the same seeds."""
import ctypes as C
import types

import numpy as np

import synth_oracle as O
from syncopy_amd import _lib
from syncopy_amd.synthdata import coupling_table

EPS32 = float(np.finfo(np.float32).eps)
_emu = _shim = None


def same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} values differ"


# ---- the emulated library and the shim ---------------------------------------------------------------------------------
def emu():
    """the library's own launchers of csrc/synth.hip on the CPU.  ctx: default limits; few: two workgroups for the tiling"""
    global _emu
    if _emu is None:
        import build_emu
        _emu = build_emu.emulated_library("synth")
        _emu.ctx, _emu.few = build_emu.ctx(_emu), build_emu.ctx(_emu, elementwise_blocks=2)
    return _emu


def shim():
    global _shim
    if _shim is None:
        import build_emu
        _shim = build_emu.build_shim("synth_route_shim.cpp", "libsynthroute.so")
        ll, out, err = C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_char_p)
        _shim.sr_ar2.restype, _shim.sr_ar2.argtypes = C.c_int, [ll, ll, ll, _lib.c_i32p, _lib.c_i32p, ll, out, err]
        _shim.sr_phase.restype, _shim.sr_phase.argtypes = C.c_int, [ll, ll, ll, out, err]
        _shim.sr_tile.restype, _shim.sr_tile.argtypes = C.c_int, [ll, ll, ll, C.c_ulonglong, ll, out, err]
        _shim.sr_max_channels.restype = C.c_int
    return _shim


def _answer(rc, out, err, names):
    if rc != 0:
        return types.SimpleNamespace(err=err.value.decode())
    return types.SimpleNamespace(err=None, **dict(zip(names, list(out))))


def route_ar2(ntrials, nsamples, nchan, rowptr, col, lds_per_block=160 * 1024):
    rowptr, col = np.ascontiguousarray(rowptr, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32)
    out, err = (C.c_longlong * 6)(), C.c_char_p()
    rc = shim().sr_ar2(ntrials, nsamples, nchan, rowptr.ctypes.data_as(_lib.c_i32p), col.ctypes.data_as(_lib.c_i32p),
                       lds_per_block, out, C.byref(err))
    return _answer(rc, out, err, ("coupled", "csr_in_lds", "block", "grid", "lds_bytes", "nnz"))


def route_phase(ntrials, nsamples, nchan):
    out, err = (C.c_longlong * 2)(), C.c_char_p()
    return _answer(shim().sr_phase(ntrials, nsamples, nchan, out, C.byref(err)), out, err, ("block", "grid"))


def route_tile(ntrials, nsamples, nchan, out_addr=1 << 40, max_blocks=4096):
    out, err = (C.c_longlong * 3)(), C.c_char_p()
    return _answer(shim().sr_tile(ntrials, nsamples, nchan, out_addr, max_blocks, out, C.byref(err)), out, err,
                   ("lane_bytes", "lanes", "grid"))


def emu_ar2_raw(noise, rowptr, col, w, alphas, ctx=None):
    """spyhip_synth_ar2 of the emulated library on NumPy arrays: (return code, out)"""
    lib = emu()
    noise = np.ascontiguousarray(noise, dtype=np.float64)
    rowptr, col = np.ascontiguousarray(rowptr, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.full(noise.shape, np.nan, dtype=np.float32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)         # noqa: E731
    rc = lib.spyhip_synth_ar2(ctx or lib.ctx, vp(noise), noise.shape[0], noise.shape[1], noise.shape[2], float(alphas[0]),
                              float(alphas[1]), rowptr.ctypes.data_as(_lib.c_i32p), col.ctypes.data_as(_lib.c_i32p),
                              vp(rowptr), vp(col), vp(w), vp(out))
    return rc, out


def emu_dev(ctx=None):
    """`dev` on the emulated library"""
    lib = emu()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)         # noqa: E731

    def ar2(noise, AdjMat, alphas):
        rc, out = emu_ar2_raw(noise, *coupling_table(AdjMat), alphas, ctx)
        assert rc == 0
        return out

    def phase(wn, lin, ps0, rel_eps, want_cos):
        wn, lin, ps0 = (np.ascontiguousarray(x, dtype=np.float32) for x in (wn, lin, ps0))
        out = np.full(wn.shape, np.nan, dtype=np.float32)
        assert lib.spyhip_synth_phase(ctx or lib.ctx, vp(wn), vp(lin), vp(ps0), float(rel_eps), wn.shape[0], wn.shape[1],
                                      wn.shape[2], int(want_cos), vp(out)) == 0
        return out

    def tile(col, ntrials, nchan):
        col = np.ascontiguousarray(col, dtype=np.float32)
        out = np.full((ntrials, col.size, nchan), np.nan, dtype=np.float32)
        assert lib.spyhip_synth_tile(ctx or lib.ctx, vp(col), ntrials, col.size, nchan, vp(out)) == 0
        return out
    return types.SimpleNamespace(ar2=ar2, phase=phase, tile=tile)


# ---- AR(2) -----------------------------------------------------------------------------------------------------------
def _dense3():
    return O.mk_RandomAdjMat(3, conn_thresh=1.0, seed=0)        # every off-diagonal entry 0.125


def _with_diagonal():
    adj = O.mk_RandomAdjMat(5, conn_thresh=0.6, seed=2)
    adj[1, 1] = 0.1
    adj[3, 3] = -0.05
    return adj


# name -> (AdjMat, alphas): stable couplings (mk_RandomAdjMat's normalisation), so that a flipped rounding decays
COUPLED = {
    "default 2 -> 1 (receiver 1 has no sender)": (None, (0.55, -0.8)),
    "3 dense": (_dense3(), (0.55, -0.8)),
    "diagonal entries": (_with_diagonal(), (0.55, -0.8)),
    "65 channels": (O.mk_RandomAdjMat(65, seed=1), (0.55, -0.8)),
    "alpha1 = 0": (_dense3(), (0.0, -0.5)),
}
UNCOUPLED = {
    "1 channel": (np.zeros((1, 1)), (0.55, -0.8)),
    "red noise": (np.diag(np.zeros(3)), [0.9, 0]),
    "65 channels": (np.zeros((65, 65)), (0.55, -0.8)),
    "diagonal only": (np.diag([0.1, 0.0, -0.2, 0.05]), (0.5, -0.3)),
}
SAMPLES = (2, 3, 67)            # no step, one step, more than a round of the load pipeline with a ragged end
TRIALS = (1, 3)


def ar2_inputs(AdjMat, nsamples, ntrials, seed=11):
    nchan = 2 if AdjMat is None else np.asarray(AdjMat).shape[0]
    seeds = O.trial_seeds(ntrials, seed)
    noise = np.stack([np.random.default_rng(s).normal(size=(nsamples, nchan)) for s in seeds])
    return noise, seeds


def ar2_expected(AdjMat, alphas, nsamples, seeds):
    return np.stack([O.ar2_network(AdjMat=AdjMat, nSamples=nsamples, alphas=alphas, seed=s) for s in seeds])


def within_ar2_bounds(got, want, what=""):
    """the coupled kernel against the oracle: |d| <= 16 eps32 RMS of the channel, and at most 1 % of the values differ at
    all (a float64 sum in another order than the BLAS's can only flip a float32 rounding, and a flip decays)"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rms = np.sqrt(np.mean(want.astype(np.float64) ** 2, axis=(0, 1)))
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    worst = float(np.max(d / (EPS32 * rms)))
    print(f"{what}: {differ} of {got.size} values differ, largest |d| = {worst:.3g} eps32 RMS")
    assert worst <= 16.0, (what, worst)
    assert differ <= 0.01 * got.size, (what, differ, got.size)


def check_ar2_coupled(dev, name, nsamples, ntrials):
    adj, alphas = COUPLED[name]
    noise, seeds = ar2_inputs(adj, nsamples, ntrials)
    got = dev.ar2(noise, np.array([[0, 0], [0.25, 0]]) if adj is None else adj, alphas)     # (None: analog.py:231-233)
    within_ar2_bounds(got, ar2_expected(adj, alphas, nsamples, seeds), f"{name}, {nsamples} samples, {ntrials} trials")
    return got


def check_ar2_uncoupled(dev, name, nsamples, ntrials):
    adj, alphas = UNCOUPLED[name]
    noise, seeds = ar2_inputs(adj, nsamples, ntrials)
    got = dev.ar2(noise, adj, alphas)
    same_bits(got, ar2_expected(adj, alphas, nsamples, seeds))
    return got


# ---- phase diffusion ---------------------------------------------------------------------------------------------------
PHASE_SAMPLES = (1, 2, 65)
PHASE_CHANNELS = (1, 65)


def phase_inputs(freq, eps, samplerate, nchan, nsamples, rand_ini, seeds):
    """what the front end hands the kernel, restated from analog.py:161-175 in NumPy-1 dtypes"""
    wn = np.stack([O.white_noise(nSamples=nsamples, nChannels=nchan, seed=s) for s in seeds])
    omega0 = 2 * np.pi * freq
    lin = np.float32(omega0) * np.linspace(0, nsamples / samplerate, nsamples, dtype="f4")
    ps0 = np.zeros((len(seeds), nchan), dtype=np.float32)
    if rand_ini:
        ps0 = np.stack([np.float32(2 * np.pi) * np.random.default_rng(s).uniform(size=nchan).astype("f4") for s in seeds])
    return wn, lin, ps0, np.sqrt(omega0 / samplerate * eps)


def check_phase(dev, nsamples, nchan, rand_ini, return_phase, ntrials=3, freq=60, eps=0.1, samplerate=1000):
    seeds = O.trial_seeds(ntrials, 5)
    wn, lin, ps0, rel_eps = phase_inputs(freq, eps, samplerate, nchan, nsamples, rand_ini, seeds)
    got = dev.phase(wn, lin, ps0, rel_eps, not return_phase)
    want = np.stack([O.phase_diffusion(freq, eps, samplerate, nchan, nsamples, rand_ini, return_phase, s) for s in seeds])
    if return_phase:
        same_bits(got, want)
    else:
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        worst = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) / EPS32
        print(f"cos, {nsamples} samples, {nchan} channels: largest |d| = {worst:.3g} eps32")
        assert worst <= 4.0, worst
    return got


# ---- tiling --------------------------------------------------------------------------------------------------------------
TILE_CHANNELS = (1, 3, 4, 65, 68)       # 4 and 68: whole 16-byte lanes
TILE_SAMPLES = (1, 130)


def check_tile(dev, nsamples, nchan, ntrials):
    for trial in (O.harmonic(30, 1000, nSamples=nsamples, nChannels=nchan), O.linear_trend(-2.5, nSamples=nsamples, nChannels=nchan)):
        got = dev.tile(trial[:, 0], ntrials, nchan)
        same_bits(got, np.stack([trial] * ntrials))
