"""The cross-spectral stage of the library on the CPU, for tests/test_emu_kernels.py and tests/test_emu_csd.py: the
emulator units tests/emu/csd_emu.cpp (csd.hip, ppc.hip) and ccov_emu.cpp (ccov.hip), called through the public ABI
(syncopy_amd._lib.SIGNATURES) on NumPy arrays.  Nothing of a route or a launch is decided here."""
import ctypes as C
import functools

import numpy as np

import build_emu
from emu_driver import OUT_KINDS

NOT_EMULATED = -101         # EMU_NOT_EMULATED (emu_unit.h): K4h, lag transforms above 8192 points
NO_RECUT = 2 ** 31 - 1      # compute units of the tests' default chip: so many that no launch is re-cut into a tail


@functools.lru_cache(None)
def lib(name="csd"):
    L = build_emu.emulated_library(name)
    if name == "csd":
        L.emu_csd_kernel_code.restype, L.emu_csd_kernel_code.argtypes = C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.emu_csd_accumulate_tpw.restype = C.c_int
        L.emu_csd_accumulate_tpw.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return L


@functools.lru_cache(None)
def ctx(name="csd", num_cu=NO_RECUT, lds_per_block=0, phase_exact=False, elementwise_blocks=0, workgroups=0):
    """a context of an emulated library (kept for the session): the chip the route plans for, spyhip_csd_set_phase_exact,
    and the two launch limits csd.hip reads"""
    c = build_emu.ctx(lib(name), elementwise_blocks=elementwise_blocks, workgroups=workgroups)
    lib(name).emu_ctx_set_chip(c, num_cu, lds_per_block)
    if phase_exact:
        assert lib(name).spyhip_csd_set_phase_exact(c, 1) == 0
    return c


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def launches():
    return build_emu.launches(lib())


def csd_accumulate(spec, acc, force_tpw=0, blocked=False, force_4m=False, num_cu=None, **limits):
    """spyhip_csd_accumulate: spec (R, F, C) complex64, acc (F, C, C) complex64 in place - spyhip_csd_accumulate_blocked
    with spec (R, ceil(C/4), F, 4) for `blocked`.  `force_4m`: a context with spyhip_csd_set_phase_exact; `num_cu`: the
    compute units the route plans for; `limits`: lowered launch limits (ctx).  `force_tpw` (1, 3, 5): csd_accum_kernel<tpw,
    tpw - 1> whatever the route says.  Returns the code of the first step of the route (csd_emu.cpp: emu_csd_kernel_code)
    after checking that the first launch is that step's: its threads and LDS bytes, and its grid where the step states one."""
    c = ctx(num_cu=num_cu or NO_RECUT, phase_exact=bool(force_4m), **limits)
    spec = np.ascontiguousarray(spec, dtype=np.complex64)
    assert acc.dtype == np.complex64 and acc.flags.c_contiguous
    R, (F, Cn) = spec.shape[0], acc.shape[:2]
    assert spec.shape == ((R, (Cn + 3) // 4, F, 4) if blocked else (R, F, Cn))
    L = lib()
    if force_tpw:
        assert not blocked and L.emu_csd_accumulate_tpw(c, ptr(spec), R, F, Cn, ptr(acc), force_tpw) == 0
        return force_tpw
    first = np.zeros(3, dtype=np.int64)
    code = L.emu_csd_kernel_code(c, R, F, Cn, int(blocked), ptr(first))
    L.emu_launch_log_reset()
    rc = (L.spyhip_csd_accumulate_blocked if blocked else L.spyhip_csd_accumulate)(c, ptr(spec), R, F, Cn, ptr(acc))
    assert rc == 0, rc
    log = build_emu.launches(L, reset=False)
    assert len(log) and tuple(log[0, [3, 6]]) == tuple(first[1:]) and first[0] in (-1, log[0, 0]), (code, first, log)
    return code


def csd_finalize(acc, scale):
    F, Cn, _ = acc.shape
    assert lib().spyhip_csd_finalize(ctx(), ptr(acc), F, Cn, scale) == 0


def coh_from_accumulator(acc, scale, output="abs"):
    """spyhip_coh_from_accumulator (raw lower-triangle accumulator -> coherence)"""
    F, Cn, _ = acc.shape
    kind = OUT_KINDS[output]
    out = np.zeros((F, Cn, Cn), dtype=np.complex64 if kind == 2 else np.float32)
    assert lib().spyhip_coh_from_accumulator(ctx(), ptr(acc), F, Cn, scale, kind, ptr(out)) == 0
    return out


def coh_normalize(csd, output="abs", elementwise_blocks=2):
    """spyhip_coh_normalize on 2 x `elementwise_blocks` workgroups at the most (0: the library's cap): four by default,
    so that the grid-stride loop runs"""
    F, Cn, _ = csd.shape
    kind = OUT_KINDS[output]
    out = np.empty((F, Cn, Cn), dtype=np.complex64 if kind == 2 else np.float32)
    assert lib().spyhip_coh_normalize(ctx(elementwise_blocks=elementwise_blocks), ptr(csd), F, Cn, kind, ptr(out)) == 0
    return out


def jack_coh_accumulate(spec, ntaper, S, direct, output, ntrials_total, sum_d, sum_d2):
    """spyhip_jack_coh_accumulate (sum_d / sum_d2 float64 in place; sum_d complex128 for 'complex')"""
    spec = np.ascontiguousarray(spec, dtype=np.complex64)
    R, F, Cn = spec.shape
    S = np.ascontiguousarray(S, dtype=np.complex64)
    direct = np.ascontiguousarray(direct)
    assert lib().spyhip_jack_coh_accumulate(ctx(), ptr(spec), R // ntaper, ntaper, F, Cn, ptr(S), ptr(direct), OUT_KINDS[output],
                                            ntrials_total, ptr(sum_d), ptr(sum_d2)) == 0


def ppc_accumulate(spec, ntaper, acc):
    """spyhip_ppc_accumulate: spec (T * ntaper, F, C) complex64, acc (F, C, C) complex64 in place"""
    spec = np.ascontiguousarray(spec, dtype=np.complex64)
    R, F, Cn = spec.shape
    assert lib().spyhip_ppc_accumulate(ctx(), ptr(spec), R // ntaper, ntaper, F, Cn, ptr(acc)) == 0


def ppc_accumulate_csd(csd, acc):
    csd = np.ascontiguousarray(csd, dtype=np.complex64)
    assert lib().spyhip_ppc_accumulate_csd(ctx(), ptr(csd), csd.shape[0], acc.size, ptr(acc)) == 0


def ppc_finalize(acc, ntrials, lower_only):
    F, ni, nj = acc.shape
    out = np.empty((F, ni, nj), dtype=np.float32)
    assert lib().spyhip_ppc_finalize(ctx(), ptr(acc), F, ni, nj, int(lower_only), ntrials, ptr(out)) == 0
    return out


def ccov_from_accumulator(acc, nsamples, scale, norm=0):
    """spyhip_ccov_from_accumulator: acc (nfft/2+1, C, C) complex64 -> (nlag, C, C) float32"""
    acc = np.ascontiguousarray(acc, dtype=np.complex64)
    F, Cn, _ = acc.shape
    out = np.zeros((nsamples // 2 + (nsamples & 1), Cn, Cn), dtype=np.float32)
    assert lib("ccov").spyhip_ccov_from_accumulator(ctx("ccov"), ptr(acc), 2 * (F - 1), Cn, nsamples, scale, norm, ptr(out)) == 0
    return out
