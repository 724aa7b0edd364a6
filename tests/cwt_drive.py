"""The wavelet plan of the library on the CPU, for tests/test_emu_kernels.py: the emulator unit tests/emu/cwt_emu.cpp
(cwt.hip), called through the public ABI (syncopy_amd._lib.SIGNATURES) on NumPy arrays, and the two pure route functions
the tests ask (tests/emu/cwt_route_shim.cpp).  Nothing of a route or a launch is decided here."""
import ctypes as C
import functools

import numpy as np

import build_emu
from cwt64_ref import cwt64_taps
from emu_driver import OUT_KINDS


@functools.lru_cache(None)
def lib():
    L = build_emu.emulated_library("cwt")
    L.emu_ctx_set_cwt_budgets.restype, L.emu_ctx_set_cwt_budgets.argtypes = None, [C.c_void_p, C.c_longlong, C.c_longlong]
    L.emu_cwt_trace.restype, L.emu_cwt_trace.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    return L


@functools.lru_cache(None)
def route():
    R = build_emu.build_shim("cwt_route_shim.cpp", "libspycwtroute.so")
    R.cwt_conv_length64.restype = C.c_longlong
    R.cwt_direct_fits.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_ulonglong, C.c_ulonglong]
    return R


def _p(a, typ=None):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p if typ is None else C.POINTER(typ))


def cwt_exec(data, seg_start, trial_lo, trial_hi, nsig, scales, dt, w0=6.0, detrend=-1, output="pow", tpos=None,
             ntime_out=None, chan_idx=None, accumulate=0, family=None, order=None, sl_cycles=None, direct=True,
             precision64=False, num_cu=None, stage_budget=None, work_budget=None, out=None, trace=None):
    """spyhip_cwt_plan_create_family + spyhip_cwt_exec.  family None (Morlet, w0) / "Paul" / "DOG" with `order`, or
    `sl_cycles` (MorletSL, k_sd = 5); `direct` / `precision64`: spyhip_cwt_plan_set_direct / _set_precision; `num_cu`,
    `stage_budget`, `work_budget` (bytes): the chip and the launch limits of the context instead of the library's;
    `out`: the array to store into / add to (a zeroed one by default); `trace`: a list that receives one line per step of the
    call (cwt_emu.cpp: emu_cwt_trace)."""
    L = lib()
    data = np.ascontiguousarray(data, dtype=np.float32)
    ld = data.shape[1]
    nchan = ld if chan_idx is None else len(chan_idx)
    ci = None if chan_idx is None else np.ascontiguousarray(chan_idx, dtype=np.int32)
    ss, tl, th = (np.ascontiguousarray(a, dtype=np.int64) for a in (seg_start, trial_lo, trial_hi))
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    fam, p0, p1 = (1, sl_cycles, 5.0) if sl_cycles is not None else ({None: 0, "Paul": 2, "DOG": 3}[family], order or w0, 0.0)
    kind = OUT_KINDS[output]
    tp = None if tpos is None else np.ascontiguousarray(tpos, dtype=np.int32)
    nto = nsig if tpos is None else int(ntime_out)
    shape = (1 if accumulate == 2 else len(ss), nto, len(sc), nchan)
    if out is None:
        out = np.zeros(shape, dtype=np.complex64 if kind == 2 else np.float32)
    assert out.shape == shape and out.flags.c_contiguous and out.dtype == (np.complex64 if kind == 2 else np.float32)
    ctx = build_emu.ctx(L)
    L.emu_ctx_set_chip(ctx, num_cu or 0, 0)
    L.emu_ctx_set_cwt_budgets(ctx, stage_budget or 0, work_budget or 0)
    plan = C.c_void_p()
    try:
        rc = L.spyhip_cwt_plan_create_family(ctx, nsig, nchan, len(sc), _p(sc, C.c_double), dt, fam, p0, p1, detrend, kind,
                                             _p(tp, C.c_int32), nto, C.byref(plan))
        assert rc == 0, rc
        if not direct:
            assert L.spyhip_cwt_plan_set_direct(plan, 0) == 0
        if precision64:
            assert L.spyhip_cwt_plan_set_precision(plan, 1) == 0
        if trace is not None:
            text = C.create_string_buffer(1 << 16)
            assert L.emu_cwt_trace(plan, len(ss), accumulate, text, len(text)) == 0
            trace.extend(text.value.decode().splitlines())
        rc = L.spyhip_cwt_exec(plan, _p(data), ld, _p(ci), _p(ss), _p(tl), _p(th), len(ss), _p(out), accumulate)
        assert rc == 0, rc
    finally:
        L.spyhip_cwt_plan_destroy(plan)
        L.emu_ctx_destroy(ctx)
    return out


def cwt_conv_length64(nsig, ntaps):
    """L of spyhip_cwt_plan_set_precision: 2^m >= max(16, nsig + the longest kernel - 1)."""
    nt = np.ascontiguousarray(ntaps, dtype=np.int32)
    return route().cwt_conv_length64(C.c_int(nsig), _p(nt, C.c_int), C.c_int(nt.size))


def cwt64_exec(data, seg_start, trial_lo, trial_hi, nsig, scales, dt, per_launch=None, seg_chunk=None, **kw):
    """cwt_exec at reference precision (cwt64_kernel.h).  `per_launch` (segment, channel) items per cwt64_kernel launch and
    `seg_chunk` segments per staging chunk, turned into the byte budgets that make the route choose them."""
    nchan = np.asarray(data).shape[1] if kw.get("chan_idx") is None else len(kw["chan_idx"])
    if per_launch:
        taps = cwt64_taps(nsig, scales, dt, kw.get("w0", 6.0), kw.get("family"), kw.get("order"), kw.get("sl_cycles"))
        kw.update(num_cu=1, work_budget=per_launch * 3 * 16 * cwt_conv_length64(nsig, [h.size for h, _ in taps]))
        assert per_launch >= 2                   # (the route launches at least two items per compute unit)
    if seg_chunk:
        kw.update(stage_budget=seg_chunk * len(scales) * nchan * nsig * (8 if OUT_KINDS[kw.get("output", "pow")] == 2 else 4))
    return cwt_exec(data, seg_start, trial_lo, trial_hi, nsig, scales, dt, precision64=True, **kw)


def cwt_direct_fits(tpos, nsig, V, rowb, chanb):
    """cwt_route.h: cwt_direct_fits - may the direct kernels write a plan with these slots, block groups and row bytes."""
    tp = None if tpos is None else np.ascontiguousarray(tpos, dtype=np.int32)
    v = np.ascontiguousarray(V, dtype=np.int32)
    return bool(route().cwt_direct_fits(_p(tp, C.c_int), nsig, _p(v, C.c_int), v.size, rowb, chanb))
