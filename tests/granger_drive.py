"""The Wilson / Granger stage of the library on the CPU, for tests/test_emu_kernels.py and tests/test_emu_granger.py: the emulator unit
tests/emu/granger_emu.cpp (granger.hip), called through the public ABI (syncopy_amd._lib.SIGNATURES) and, for launchers
without a public entry point, through the unit's pointer-passing entries, on NumPy arrays.  What a launch should look
like - kernel name, grid, threads, LDS bytes - is asked of the route (tests/emu/granger_route_shim.cpp) for the
launcher's arguments and compared with the launch log; nothing of a route or a launch is decided here."""
import ctypes as C
import functools
import types

import numpy as np

import build_emu

vp = C.c_void_p


@functools.lru_cache(None)
def lib():
    L = build_emu.emulated_library("granger")
    ll, i = C.c_longlong, C.c_int
    for name, args in (("emu_w_gemm", [vp, vp, vp, vp, i, i, ll, ll, ll, i, i, vp]),
                       ("emu_w_fused_check", [vp, vp, vp, i, i, vp, vp]),
                       ("emu_w_inv", [vp, vp, vp, i, i, vp, i]),
                       ("emu_w_chol", [vp, vp, i, i, vp]),
                       ("emu_w_skew", [vp, vp, vp, vp, i]),
                       ("emu_w_plus_generic", [vp, vp, i, ll, vp, vp])):
        getattr(L, name).restype, getattr(L, name).argtypes = i, args
    return L


@functools.lru_cache(None)
def route():
    return build_emu.build_shim("granger_route_shim.cpp", "libspygrangerroute.so")


@functools.lru_cache(None)
def ctx(num_cu=0, lds_per_block=0):
    """a context of the emulated library (kept for the session); the chip the launchers plan for where given"""
    c = build_emu.ctx(lib(), elementwise_blocks=4)          # (relerr_kernel strides: 4 workgroups instead of 1024)
    lib().emu_ctx_set_chip(c, num_cu, lds_per_block)
    return c


def chip(num_cu=0, lds_per_block=0):
    """(compute units, LDS bytes per workgroup) of ctx(...): the library's defaults unless given"""
    return num_cu or 256, lds_per_block or 160 * 1024


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def _ask(fn, nout, *args):
    out, name = (C.c_longlong * nout)(), C.create_string_buffer(64)
    fn(*args, out, name, 64)
    return list(out), name.value.decode()


def _launched(kernel, name, grid, threads, lds):
    """the first launch since the reset is the route's: its name is `kernel` where the test names one"""
    assert kernel is None or name == kernel, (name, kernel)
    log = build_emu.launches(lib())
    assert tuple(log[0]) == (*grid, threads, 1, 1, lds), (name, log[0], grid, threads, lds)


def _batch(M):
    return (M.shape[0], M.shape[1]) if M.ndim == 3 else (1, M.shape[0])


def gemm(A, B, opB=0, addI=0, badd=None, ref=None, kernel=None):
    """A op(B) (+ I) through the library's product launcher.  n >= 48 only: `badd` (n, n) joins op(B); with `ref` (A is B,
    opB = 1) the return value is max |ref - A A^H| / |ref| of the library's fused check and no product is stored.
    `kernel`: the kernel name the route must give."""
    A = np.ascontiguousarray(A, dtype=np.complex128)
    B = np.ascontiguousarray(B, dtype=np.complex128)
    batch, n = _batch(A)
    sB = 0 if B.ndim == 2 and A.ndim == 3 else n * n
    ba = None if badd is None else np.ascontiguousarray(badd, dtype=np.complex128)
    same = A.ctypes.data == B.ctypes.data and sB == n * n
    o, name = _ask(route().wr_gemm, 10, n, batch, opB, int(same), int(ba is not None), int(ref is not None))
    L = lib()
    L.emu_launch_log_reset()
    if ref is not None:
        assert same and opB == 1
        rf = np.ascontiguousarray(ref, dtype=np.complex128)
        bigpart, part = np.full(o[7] * batch + 1, -1.0), np.full(1, -1.0)
        assert L.emu_w_fused_check(ctx(), ptr(A), ptr(rf), n, batch, ptr(bigpart), ptr(part)) == 0
        out = float(part[0])
    else:
        out = np.zeros_like(A)
        assert L.emu_w_gemm(ctx(), ptr(A), ptr(B), ptr(out), n, batch, n * n, sB, n * n, opB, addI, ptr(ba)) == 0
    _launched(kernel, name, o[2:5], o[5], o[6])
    return out


def skew(g0):
    g0 = np.ascontiguousarray(g0, dtype=np.complex128)
    S, g0S = np.zeros_like(g0), np.zeros_like(g0)
    assert lib().emu_w_skew(ctx(), ptr(g0), ptr(S), ptr(g0S), g0.shape[0]) == 0
    return S, g0S


def inv(M, blocked=False, lds_per_block=0, kernel=None):
    """The library's inverse launcher for (n, blocked) on a chip with `lds_per_block` bytes of LDS, out of place from a
    copy of the input as the Wilson iteration calls it (M is overwritten first, so a kernel that read M instead of its
    source would show); `kernel`: the name the route must give."""
    M = np.array(M, dtype=np.complex128, order="C")
    batch, n = _batch(M)
    info = np.zeros(batch, dtype=np.int32)
    src = M.copy()
    M[...] = -777.0 - 777.0j
    o, name = _ask(route().wr_inv, 4, n, int(bool(blocked)), 1, C.c_ulonglong(chip(0, lds_per_block)[1]))
    L = lib()
    L.emu_launch_log_reset()
    assert L.emu_w_inv(ctx(0, lds_per_block), ptr(M), ptr(src), n, batch, ptr(info), int(bool(blocked))) == 0
    _launched(kernel, name, (batch, 1, 1), o[1], o[2])
    return M, info


def chol(M, kernel=None):
    M = np.array(M, dtype=np.complex128, order="C")
    batch, n = _batch(M)
    info = np.zeros(batch, dtype=np.int32)
    o, name = _ask(route().wr_chol, 3, n, C.c_ulonglong(chip()[1]))
    L = lib()
    L.emu_launch_log_reset()
    assert L.emu_w_chol(ctx(), ptr(M), n, batch, ptr(info)) == 0
    _launched(kernel, name, (batch, 1, 1), o[1], o[2])
    return M, info


def plus(g, generic=False, kernel=None):
    """spyhip_wilson_plus on a half spectrum g (F, n, n) complex128 -> (gp (F, n, n), g0 (n, n)); `generic`: plus_kernel
    (the radix-4 passes in LDS) whatever the length."""
    g = np.ascontiguousarray(g, dtype=np.complex128)
    F, n, _ = g.shape
    gp = np.zeros_like(g)
    g0 = np.zeros((n, n), dtype=np.complex128)
    L = lib()
    L.emu_launch_log_reset()
    if generic:
        assert kernel == "spywil::plus_kernel"
        assert L.emu_w_plus_generic(ctx(), ptr(g), F, n * n, ptr(gp), ptr(g0)) == 0, f"no radix schedule for F = {F}"
        return gp, g0
    o, name = _ask(route().wr_plus, 7, 2 * (F - 1), C.c_longlong(n * n), C.c_ulonglong(chip()[1]), chip()[0])
    assert L.spyhip_wilson_plus(ctx(), ptr(g), F, n * n, ptr(gp), ptr(g0)) == 0, f"no radix schedule for F = {F}"
    _launched(kernel, name, (o[2], 1, 1), o[3], o[4])
    return gp, g0


def cond(A):
    """spyhip_wilson_cond of the matrices A (F, n, n), rounded to complex64 as the entry point takes them, eps = 0"""
    A64 = np.ascontiguousarray(A, dtype=np.complex64)
    F, n, _ = A64.shape
    wide, work, out = np.zeros((F, n, n), np.complex128), np.zeros((3, F, n, n), np.complex128), C.c_double()
    assert lib().spyhip_wilson_cond(ctx(), ptr(A64), F, n, 0.0, ptr(wide), ptr(work), C.byref(out)) == 0
    return out.value


def zinv(src, dst=None):
    """spyhip_zinv of src (batch, n, n) complex128 into dst (src itself: in place) -> return code"""
    batch, n, _ = src.shape
    return lib().spyhip_zinv(ctx(), ptr(src), ptr(src if dst is None else dst), batch, n)


def granger(csd64, rtol=5e-6, niter=100, cond_max=1e4, eps_max=1e-1, rc=0):
    """spyhip_granger: csd64 (F, n, n) complex64 -> (granger float32, H, Sigma, info[4]); `rc`: the return code expected
    (the arrays are meaningless after a refusal)"""
    csd64 = np.ascontiguousarray(csd64, dtype=np.complex64)
    F, n, _ = csd64.shape
    G, H, Sigma = np.zeros((F, n, n), np.float32), np.zeros((F, n, n), np.complex128), np.zeros((n, n), np.complex128)
    info = np.zeros(4)
    got = lib().spyhip_granger(ctx(), ptr(csd64), F, n, rtol, niter, cond_max, eps_max, ptr(G), ptr(H), ptr(Sigma),
                               info.ctypes.data_as(C.POINTER(C.c_double)))
    assert got == rc, (got, rc)
    return G, H, Sigma, info


def last_iterations():
    return lib().spyhip_granger_last_iterations(ctx())


def sharded_prims():
    """HipPrims of syncopy_amd/connectivity/wilson_sharded.py bound to the emulated library and host tensors: the same
    calls of the spyhip_wilson_* entry points, so granger_sharded drives the stepped sequence as it does on the device"""
    import torch
    from syncopy_amd.connectivity.wilson_sharded import HipPrims

    def check(rc, name):
        raise RuntimeError(f"{name} -> {rc}")
    prims = HipPrims.__new__(HipPrims)
    prims.be = types.SimpleNamespace(check=check)
    prims.ctx = types.SimpleNamespace(lib=lib(), handle=ctx(), bind_stream=lambda: None)
    prims.dev, prims._work = torch.device("cpu"), None
    return prims
