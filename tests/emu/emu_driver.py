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


def cwt_exec(data, seg_start, trial_lo, trial_hi, nsig, scales, dt, w0=6.0, detrend=-1, output="pow", tpos=None,
             ntime_out=None, chan_idx=None, accumulate=0, family=None, order=None, sl_cycles=None, direct=True,
             precision64=False, num_cu=None, stage_budget=None, work_budget=None, out=None, trace=None):
    """Emulated spyhip_cwt_plan_create* + spyhip_cwt_exec: the emulator samples the taps, asks the route of
    syncopy_amd/csrc/cwt_route.h for the plan and the steps, and walks them.  family None (Morlet, w0) / "Paul" / "DOG" with
    `order`, or `sl_cycles` (MorletSL, k_sd = 5); `direct` / `precision64`: spyhip_cwt_plan_set_direct / _set_precision;
    `num_cu`, `stage_budget`, `work_budget` (bytes): what the route plans for instead of the chip and the library's budgets;
    `out`: the array to store into / add to (a zeroed one by default); `trace`: a list that receives one line per step."""
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
    text = C.create_string_buffer(1 << 16)
    rc = lib().emu_cwt(_p(data, C.c_float), C.c_longlong(ld), _p(ci, C.c_int), _p(ss, C.c_longlong), _p(tl, C.c_longlong),
                       _p(th, C.c_longlong), C.c_int(len(ss)), C.c_int(nsig), C.c_int(nchan), C.c_int(len(sc)),
                       _p(sc, C.c_double), C.c_double(dt), C.c_int(fam), C.c_double(p0), C.c_double(p1), C.c_int(detrend),
                       C.c_int(kind), _p(tp, C.c_int), C.c_int(nto), out.ctypes.data_as(C.c_void_p), C.c_int(accumulate),
                       C.c_int(direct), C.c_int(precision64), C.c_longlong(num_cu or 0), C.c_longlong(stage_budget or 0),
                       C.c_longlong(work_budget or 0), text, C.c_int(len(text)))
    assert rc == 0, rc
    if trace is not None:
        trace.extend(text.value.decode().splitlines())
    return out


def cwt64_taps(nsig, scales, dt, w0=6.0, family=None, order=None, sl_cycles=None):
    """The sampled kernels of spyhip_cwt_plan_create trimmed to the taps that can overlap a signal of nsig samples, and
    each trimmed kernel's "same" offset: [(taps, centre)].  family None / "Paul" / "DOG" as O.cwt_kernel; `sl_cycles`:
    MorletSL (O.cwt_sl)."""
    from oracle import spy_oracle as O
    out = []
    for s in scales:
        if sl_cycles is None:
            h = O.cwt_kernel(s, dt, w0, family, order)
        else:
            M = 10 * s * sl_cycles / dt
            t = np.arange((-M + 1) / 2.0, (M + 1) / 2.0) * dt
            h = dt ** 0.5 / (4 * np.pi) * O.morlet_sl(t, s, sl_cycles)
        h = np.asarray(h, dtype=np.complex128)
        c = (h.size - 1) // 2
        m0, m1 = max(0, c - (nsig - 1)), min(h.size, c + nsig)
        out.append((h[m0:m1], c - m0))
    return out


def cwt_conv_length64(nsig, ntaps):
    """L of spyhip_cwt_plan_set_precision: 2^m >= max(16, nsig + the longest kernel - 1)."""
    nt = np.ascontiguousarray(ntaps, dtype=np.int32)
    f = lib().emu_cwt_conv_length64
    f.restype = C.c_longlong
    return f(C.c_int(nsig), _p(nt, C.c_int), C.c_int(nt.size))


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
    f = lib().emu_cwt_direct_fits
    f.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_ulonglong, C.c_ulonglong]
    return bool(f(_p(tp, C.c_int), nsig, _p(v, C.c_int), v.size, rowb, chanb))


# ---------------------------------------------------------------- Wilson / Granger (the sequence of spyhip_granger, granger.hip)
# Every kernel choice below is the one of syncopy_amd/csrc/granger_route.h, taken by the emulator entry itself.
LDS_PER_BLOCK = 160 * 1024          # sharedMemPerBlockOptin of the MI355X
NUM_CU = 256


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _named(kernel, name):
    if kernel is not None:
        assert name.value.decode() == kernel, (name.value.decode(), kernel)


def w_gemm(A, B, opB=0, addI=0, badd=None, ref=None, kernel=None):
    """A op(B) (+ I) through the product kernel of the route.  n >= 48 only: `badd` (n, n) joins op(B); with `ref` the
    return value is max |ref - A op(B)| / |ref| and no product is stored.  `kernel`: the kernel name the route must give."""
    A = np.ascontiguousarray(A, dtype=np.complex128)
    B = np.ascontiguousarray(B, dtype=np.complex128)
    batch, n = (A.shape[0], A.shape[1]) if A.ndim == 3 else (1, A.shape[0])
    sB = 0 if B.ndim == 2 and A.ndim == 3 else n * n
    out = np.zeros_like(A)
    ba = None if badd is None else np.ascontiguousarray(badd, dtype=np.complex128)
    rf = None if ref is None else np.ascontiguousarray(ref, dtype=np.complex128)
    name = C.create_string_buffer(64)
    lib().emu_w_gemm.restype = C.c_double
    err = lib().emu_w_gemm(_dp(A), _dp(B), _dp(out), C.c_int(n), C.c_int(batch), C.c_longlong(n * n), C.c_longlong(sB),
                           C.c_longlong(n * n), C.c_int(opB), C.c_int(addI), _dp(ba), _dp(rf), name)
    _named(kernel, name)
    return err if ref is not None else out


def w_skew(g0):
    g0 = np.ascontiguousarray(g0, dtype=np.complex128)
    n = g0.shape[0]
    S, g0S = np.zeros_like(g0), np.zeros_like(g0)
    lib().emu_w_skew(_dp(g0), _dp(S), _dp(g0S), C.c_int(n))
    return S, g0S


def w_inv(M, blocked=False, lds_per_block=LDS_PER_BLOCK, kernel=None):
    """The inverse kernel the route gives for (n, blocked, lds_per_block); `kernel`: the name it must have."""
    M = np.array(M, dtype=np.complex128, order="C")
    batch, n = (M.shape[0], M.shape[1]) if M.ndim == 3 else (1, M.shape[0])
    info = np.zeros(batch, dtype=np.int32)
    name = C.create_string_buffer(64)
    lib().emu_w_inv(_dp(M), C.c_int(n), C.c_int(batch), _dp(info), C.c_int(bool(blocked)), C.c_ulonglong(lds_per_block), name)
    _named(kernel, name)
    return M, info


def w_plus(g, generic=False, kernel=None):
    """Emulated plus operator on a half spectrum g (F, n, n) complex128 -> (gp (F, n, n), g0 (n, n)) on the kernel family
    of the route; `generic`: plus_kernel (the radix-4 passes in LDS) whatever the length."""
    g = np.ascontiguousarray(g, dtype=np.complex128)
    F, n, _ = g.shape
    L = 2 * (F - 1)
    tw = np.ascontiguousarray(np.exp(-2j * np.pi * np.arange(L) / L))
    gp = np.zeros_like(g)
    g0 = np.zeros((n, n), dtype=np.complex128)
    name = C.create_string_buffer(64)
    rc = lib().emu_w_plus(_dp(g), C.c_int(F), C.c_int(n), _dp(tw), _dp(gp), _dp(g0), C.c_ulonglong(LDS_PER_BLOCK),
                          C.c_int(NUM_CU), C.c_int(bool(generic)), name)
    assert rc == 0, f"no radix schedule for F = {F}"
    _named(kernel, name)
    return gp, g0


def w_chol(M, kernel=None):
    M = np.array(M, dtype=np.complex128, order="C")
    batch, n = (M.shape[0], M.shape[1]) if M.ndim == 3 else (1, M.shape[0])
    info = np.zeros(batch, dtype=np.int32)
    name = C.create_string_buffer(64)
    lib().emu_w_chol(_dp(M), C.c_int(n), C.c_int(batch), _dp(info), C.c_ulonglong(LDS_PER_BLOCK), name)
    _named(kernel, name)
    return M, info


def w_cond(A, iters=400):
    F, n, _ = A.shape
    Ai, info = w_inv(A)
    l1, l2 = np.zeros(F), np.zeros(F)
    lib().emu_w_power(_dp(np.ascontiguousarray(A)), C.c_int(n), C.c_int(F), C.c_int(iters), _dp(l1))
    lib().emu_w_power(_dp(Ai), C.c_int(n), C.c_int(F), C.c_int(iters), _dp(l2))
    c = l1 * l2
    c[info != 0] = np.inf
    return float(np.nanmax(np.where(np.isnan(c), np.inf, c)))


def w_err_route(n, F, forced=False):
    """(fused, subset first, subset bins) of the convergence check (granger_route.h: err_route)."""
    out = (C.c_int * 3)()
    lib().emu_w_err_route(C.c_int(n), C.c_int(F), C.c_int(bool(forced)), out)
    return bool(out[0]), bool(out[1]), out[2]


def granger(csd64, rtol=5e-6, niter=100, cond_max=1e4, eps_max=1e-1, cond_iters=400):
    """Emulated spyhip_granger: csd64 (F, n, n) complex64 -> (granger float32, H, Sigma, info[4])."""
    csd64 = np.ascontiguousarray(csd64, dtype=np.complex64)
    F, n, _ = csd64.shape

    def widen(eps):
        out = np.zeros((F, n, n), dtype=np.complex128)
        lib().emu_w_widen(_dp(csd64), _dp(out), C.c_int(n), C.c_longlong(F * n * n), C.c_double(eps))
        return out
    A = widen(0.0)
    cond0 = w_cond(A, cond_iters)
    factor = 0.0
    if not cond0 < cond_max:
        factor = -1.0
        for s in range(15):
            eps = 10.0 ** (-10.0 + (np.log10(eps_max) + 10.0) * s / 14)
            A = widen(eps)
            if w_cond(A, cond_iters) < cond_max:
                factor = eps
                break
    U, info = w_chol(A)
    assert not info.any()
    g0m = np.zeros((n, n), dtype=np.complex128)
    lib().emu_w_gamma0(_dp(A), C.c_int(F), C.c_int(n), _dp(g0m))
    Lc, info = w_chol(g0m)
    psi0_first = np.ascontiguousarray(Lc.T)
    fused, subset_first, Fs = w_err_route(n, F)
    converged, err, subset_only = False, np.inf, False

    def check(bins):          # the fused check over the bins `bins` of psi
        return w_gemm(psi[bins], psi[bins], opB=1, ref=A[bins])
    for blocked in (True, False):       # the block inverse first; a tiny pivot anywhere restarts with the pivoted kernel
        psi0 = psi0_first.copy()
        psi = np.ascontiguousarray(np.tile(psi0, (F, 1, 1)))
        tiny = False
        for _ in range(niter):
            pinv, flags = w_inv(psi, blocked=blocked)
            T2 = w_gemm(pinv, U, addI=2 if n >= 48 else 0)
            g = w_gemm(T2, T2, opB=1, addI=1)
            gp, g0 = w_plus(g)
            if fused:
                S, g0S = w_skew(g0)
                psi = w_gemm(psi, gp, badd=S)
            else:
                g0S = np.zeros((n, n), dtype=np.complex128)
                lib().emu_w_addS(_dp(gp), _dp(g0), _dp(g0S), C.c_int(F), C.c_int(n))
                psi = w_gemm(psi, gp)
            psi0 = w_gemm(psi0, g0S)
            subset_only = False
            if subset_first:
                err = check(slice(0, None, 8))
                subset_only = bool(err >= rtol or err != err)
            if fused:
                if not subset_only:
                    err = check(slice(None))
            else:
                rec = w_gemm(psi, psi, opB=1)
                lib().emu_w_relerr.restype = C.c_double
                err = lib().emu_w_relerr(_dp(A), _dp(rec), C.c_longlong(F * n * n))
            tiny = bool((flags == 2).any())
            if tiny:
                break
            if err < rtol:
                converged = True
                break
        if not tiny:
            break
    if not converged and subset_only:
        err = check(slice(None))
    Sigma = w_gemm(psi0, psi0, opB=1)
    p0i, flags = w_inv(psi0, blocked=True)
    if flags[0]:
        p0i, _i = w_inv(psi0)
    H = w_gemm(psi, p0i)
    G = np.zeros((F, n, n), dtype=np.float32)
    lib().emu_w_granger(_dp(A), _dp(H), _dp(np.ascontiguousarray(Sigma)), C.c_int(F), C.c_int(n), _dp(G))
    return G, H, Sigma, np.array([float(converged), err, factor, cond0])
