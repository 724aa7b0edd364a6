"""ctypes front end of the CPU emulation of the HIP kernels (TEST INFRASTRUCTURE ONLY).

Marshals host arrays into the entries of tests/emu/emu_kernels.cpp so that a test
can run one kernel configuration and compare it with the oracle.  Routes, tables
and launch geometry are the library's own headers on the C side; none of them is
restated here.  Never imported by the package.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import build_emu  # noqa: E402

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_emu.build())
    return _lib


def _p(a, typ):
    return None if a is None else a.ctypes.data_as(C.POINTER(typ))


OUT_KINDS = {"pow": 0, "abs": 1, "fourier": 2, "complex": 2, "real": 3, "imag": 4, "angle": 5,
             "absreal": 6, "absimag": 7}

# `force` of emu_fft_exec (emu_kernels.cpp: enum Force): the filler of one family in place of the route's choice
FORCE = {"route": 0, "generic": 1, "long": 2, "blue": 3, "mixed": 4, "declong": 5, "dec": 6,
         "dec64": 7, "half64": 8, "plain64": 9}
NO_INSTANCE = -100     # the route chose a kernel the emulator holds no instance of
LAST_KERNEL = ""       # kernel_name of the route the last call ran (spyhip_fft_plan_kernel_name)
LAST_MIXED = {}        # the schedule of the last call that ran the mixed-radix engine


def _segments(data, seg_start, seg_lo, seg_hi, chan_idx):
    """The exec arguments of spyhip_fft_exec on host arrays: data, ld, nchan, chan_idx, seg_start, seg_lo, seg_hi."""
    data = np.ascontiguousarray(data, dtype=np.float32)
    ci = None if chan_idx is None else np.ascontiguousarray(chan_idx, dtype=np.int32)
    nchan = data.shape[1] if ci is None else len(ci)
    return (data, data.shape[1], nchan, ci, np.ascontiguousarray(seg_start, dtype=np.int64),
            np.ascontiguousarray(seg_lo, dtype=np.int64), np.ascontiguousarray(seg_hi, dtype=np.int64))


def _exec(data, seg_start, seg_lo, seg_hi, nsig, nfft, tapers, scale, detrend, demean_taper, freq_idx, output, keeptapers,
          chan_idx, precision64=False, ref_mean=0, blocked=False, force="route", variant=0, nostage=False):
    """emu_fft_exec: an emulated spyhip_fft_plan_create + options + spyhip_fft_exec.  The C side asks the library's route,
    builds the library's tables and walks the library's steps; nothing about the plan is decided or built here."""
    global LAST_KERNEL
    data, ld, nchan, ci, ss, sl, sh = _segments(data, seg_start, seg_lo, seg_hi, chan_idx)
    nseg, K = len(ss), tapers.shape[0]
    tp = np.ascontiguousarray(tapers, dtype=np.float64)
    fi = None if freq_idx is None else np.ascontiguousarray(freq_idx, dtype=np.int32)
    nfsel = nfft // 2 + 1 if fi is None else len(fi)
    kind = OUT_KINDS[output]
    kout = K if keeptapers else 1
    out = np.full((nseg, kout, nfsel, nchan), np.nan, dtype=np.complex64 if kind == 2 else np.float32)
    if blocked:
        assert kind == 2 and keeptapers
        out = np.full((nseg * kout, (nchan + 3) // 4, nfsel, 4), np.nan, dtype=np.complex64)
    name = C.create_string_buffer(256)
    info = np.zeros(8, dtype=np.int32)
    rc = lib().emu_fft_exec(
        C.c_int(nsig), C.c_int(nfft), C.c_int(nchan), C.c_int(K), _p(tp, C.c_double), C.c_double(scale), C.c_int(detrend),
        C.c_int(int(demean_taper)), _p(fi, C.c_int), C.c_int(nfsel), C.c_int(kind), C.c_int(int(keeptapers)),
        C.c_int(int(precision64)), C.c_int(ref_mean), C.c_int(int(blocked)), C.c_int(FORCE[force]), C.c_int(int(variant)),
        C.c_int(int(nostage)), _p(data, C.c_float), C.c_longlong(ld), _p(ci, C.c_int), _p(ss, C.c_longlong),
        _p(sl, C.c_longlong), _p(sh, C.c_longlong), C.c_int(nseg), out.ctypes.data_as(C.c_void_p), name, C.c_int(256),
        _p(info, C.c_int))
    LAST_KERNEL = name.value.decode()
    if rc == NO_INSTANCE:
        raise NotImplementedError(f"the emulator holds no instance of {LAST_KERNEL!r} (nfft={nfft}, force={force}, {variant})")
    if rc != 0:
        raise RuntimeError(f"emu_fft_exec(nfft={nfft}, force={force}, {variant}) -> {rc}")
    if LAST_KERNEL.startswith("mtmfft_mixed_kernel"):
        LAST_MIXED.update(dict(zip(("G", "th", "npass", "stage", "threads", "radix0", "radix_last"),
                                   (int(v) for v in info[1:]))), nfft=nfft)
    return out, int(info[1])


def fft_exec(data, seg_start, seg_lo, seg_hi, nsig, nfft, tapers, scale, detrend=-1, demean_taper=False,
             freq_idx=None, output="pow", keeptapers=True, chan_idx=None, G=None, force_generic=False, blocked=False,
             force_long=False, reference_mean=False, no_mixed=False, mixed_nostage=False, dec=None, mixed=False):
    """Emulated spyhip_fft_exec.  data: (rows, ld) float32; tapers: (K, nsig) float64.  Without a forcing keyword the
    kernel family is the one spyfft::fft_route gives the shape; LAST_KERNEL names it.
    blocked: channel-blocked hand-over layout (nseg*K, ceil(nchan/4), nfsel, 4) (fourier, keeptapers).
    reference_mean: constant detrending with the means of seq_mean_kernel (spyhip_fft_plan_set_reference_mean).
    Forcing keywords (the filler of that family in mtmfft_route.h, whatever the route says): force_generic (the library's
    SPYHIP_FORCE_GENERIC), force_long, no_mixed (Bluestein on the packed engine), mixed, dec (id of a compile-time
    schedule of emu_kernels.cpp: run_dec_id; < 0: the HALF form).  mixed_nostage: the re-read path of the mixed engine.
    G: the quads per workgroup the caller expects of the route; another value is an error."""
    forced = [k for k, on in (("dec", dec is not None), ("generic", force_generic), ("long", force_long), ("blue", no_mixed),
                              ("mixed", mixed)) if on]
    assert len(forced) <= 1, forced
    out, g = _exec(data, seg_start, seg_lo, seg_hi, nsig, nfft, tapers, scale, detrend, demean_taper, freq_idx, output,
                   keeptapers, chan_idx, ref_mean=int(bool(reference_mean)), blocked=blocked,
                   force=forced[0] if forced else "route", variant=0 if dec is None else dec, nostage=mixed_nostage)
    if G is not None and G != g:
        raise ValueError(f"G={G}: the route launches {LAST_KERNEL!r} with {g} quads per workgroup")
    return out


def fft_exec_f64(data, seg_start, seg_lo, seg_hi, nsig, nfft, tapers, scale, detrend=-1, demean_taper=False,
                 freq_idx=None, output="pow", keeptapers=True, chan_idx=None, reference_mean=False, seg_f64=False,
                 dec=None, bluestein=None, emu_id=None):
    """Emulated spyhip_fft_exec of a plan with spyhip_fft_plan_set_precision(plan, 1); the family is the one
    spyfft::fft_route64 gives the length unless forced: dec=True - the compile-time schedule of mtmfft_dec64_kernel for
    this nfft, dec="half" - its HALF form (single channels through the schedule of nfft / 2; `emu_id` picks a variant that
    shares its nfft with another, 2002), bluestein=False - the any-length kernel without the chirp-z form."""
    force, variant = "route", 0
    if dec == "half":
        force, variant = "half64", -(emu_id or nfft)
    elif dec:
        force, variant = "dec64", nfft
    elif bluestein is False:
        force = "plain64"
    out, _ = _exec(data, seg_start, seg_lo, seg_hi, nsig, nfft, tapers, scale, detrend, demean_taper, freq_idx, output,
                   keeptapers, chan_idx, precision64=True, ref_mean=2 if seg_f64 else int(bool(reference_mean)),
                   force=force, variant=variant)
    if bluestein:
        assert "Bluestein" in LAST_KERNEL, LAST_KERNEL
    return out


def fft_exec_declong(data, seg_start, seg_lo, seg_hi, nsig, P, M, tapers, scale, detrend=-1, demean_taper=False, freq_idx=None,
                     output="pow", keeptapers=True, chan_idx=None, reference_mean=False):
    """Emulated spyhip_fft_exec of a K1L2 plan (mtmfft_declong.h), forced: nfft = P M, split as the route splits it."""
    out, _ = _exec(data, seg_start, seg_lo, seg_hi, nsig, P * M, tapers, scale, detrend, demean_taper, freq_idx, output,
                   keeptapers, chan_idx, ref_mean=int(bool(reference_mean)), force="declong")
    assert LAST_KERNEL.startswith(f"declong<{P} x {M},"), LAST_KERNEL
    return out


def seq_mean(data, seg_start, seg_lo, seg_hi, nsig, chan_idx=None):
    """Emulated seq_mean_kernel: (nseg, nchan) float32 means in the reference's summation order."""
    data, ld, nchan, ci, ss, sl, sh = _segments(data, seg_start, seg_lo, seg_hi, chan_idx)
    means = np.full((len(ss), nchan), np.nan, dtype=np.float32)
    lib().emu_seq_mean(_p(data, C.c_float), C.c_longlong(ld), _p(ci, C.c_int), _p(ss, C.c_longlong),
                       _p(sl, C.c_longlong), _p(sh, C.c_longlong), C.c_int(len(ss)), C.c_int(nsig), C.c_int(nchan),
                       _p(means, C.c_float))
    return means
