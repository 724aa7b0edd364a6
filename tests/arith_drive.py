"""What the CPU emulation (tests/test_arith.py) and the GPU tests (tests/test_gpu_arith.py) of the operator arithmetic
share: the emulator's driver, the comparison rules, the inputs aimed at the kernel's dispatch edges and the parity checks
of the issue, written against a function `apply(x, operand, operator, reflected) -> array` that either side supplies."""
import ctypes as C
import types

import numpy as np

from syncopy_amd import _lib

OP = {"add": 0, "sub": 1, "mul": 2, "div": 3, "rsub": 4, "rdiv": 5, "pow": 6, "square": 7, "copy": 8, "ones": 9, "sqrt": 10}
TYPE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.complex64): 2, np.dtype(np.complex128): 3}
# the nine base -> result pairs of csrc/arith.hip
PAIRS = [("f4", "f4"), ("f4", "f8"), ("f4", "c8"), ("f4", "c16"), ("f8", "f8"), ("f8", "c16"), ("c8", "c8"), ("c8", "c16"),
         ("c16", "c16")]

_emu = None


def emu():
    """the library's own launcher of csrc/arith.hip on the CPU.  ctx: default launch limits; few: two workgroups"""
    global _emu
    if _emu is None:
        import build_emu
        _emu = build_emu.emulated_library("arith")
        _emu.ctx, _emu.few = build_emu.ctx(_emu), build_emu.ctx(_emu, elementwise_blocks=2)
    return _emu


def view(array_shape, inner):
    """the broadcast view of spyhip_arith (what backend.arith_view computes, written out again for the emulator)"""
    shape = (1,) * (1 + len(inner) - len(array_shape)) + tuple(array_shape)
    shape = shape[:1] + (1,) * (3 - len(inner)) + shape[1:]
    inner = (1,) * (3 - len(inner)) + tuple(inner)
    assert len(shape) == 4 and all(s in (1, e) for s, e in zip(shape[1:], inner))
    stride, acc = [0] * 4, 1
    for i in (3, 2, 1, 0):
        stride[i], acc = (acc if shape[i] > 1 else 0), acc * shape[i]
    return np.array((shape[0],) + inner, dtype=np.int64), np.array(stride, dtype=np.int64)


def emu_arith(op, a, desc, out, scalar=0.0, array=None, operand=None, chan=None, ctx=None):
    """spyhip_arith of the emulated library on NumPy arrays (the arguments of backend.arith); returns its return code"""
    lib = emu()
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)              # noqa: E731
    i64 = lambda x: None if x is None else x.ctypes.data_as(_lib.c_i64p)             # noqa: E731
    desc = np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, 4)
    assert a.flags.c_contiguous and out.flags.c_contiguous
    extent = stride = b = None
    b_rows = mode = 0
    if array is not None:
        assert array.dtype == out.dtype and array.flags.c_contiguous
        (extent, stride), b, b_rows, mode = view(array.shape, out.shape[1:]), array, array.size, 1
    elif operand is not None:
        assert operand.dtype == out.dtype and operand.flags.c_contiguous
        b, b_rows, mode = operand, operand.shape[0], 2
    chan_h = None if chan is None else np.ascontiguousarray(chan, dtype=np.int32)
    width = int(np.prod(out.shape[1:], dtype=np.int64))
    return lib.spyhip_arith(ctx or lib.ctx, OP[op], mode, TYPE[a.dtype], TYPE[out.dtype], ptr(a), a.shape[0], ptr(b), b_rows,
                            i64(extent), i64(stride), float(np.real(scalar)), float(np.imag(scalar)), i64(desc), ptr(desc),
                            desc.shape[0], width, None if chan_h is None else chan_h.ctypes.data_as(_lib.c_i32p),
                            ptr(chan_h), out.shape[-1], a.shape[-1], ptr(out), out.shape[0])


def emu_run(ctx=None):
    """a stand-in for arithmetic._run that computes a plan of the front end with the emulated library"""
    def table(src, starts, brow):
        n = [b - a for a, b in src.rows]
        return np.stack([starts, [a for a, _ in src.rows], brow, n], axis=1)

    def run(plan, out):
        res = np.empty((plan.nrows,) + plan.inner, dtype=plan.opres)
        src = types.SimpleNamespace(rows=plan.rows, chans=plan.chans)
        host = np.ascontiguousarray(plan.base.data)
        kw, brow = {}, plan.starts
        if plan.mode == "scalar":
            kw = {"scalar": plan.scalar}
        elif plan.mode == "array":
            kw = {"array": plan.array}
        else:
            other = plan.other
            b = np.empty_like(res)
            assert emu_arith("copy", np.ascontiguousarray(other.base.data), table(other, plan.starts, plan.starts), b,
                             chan=other.chans, ctx=ctx) == 0
            kw = {"operand": b}
        assert emu_arith(plan.op, host, table(src, plan.starts, brow), res, chan=plan.chans, ctx=ctx, **kw) == 0
        out.data = res
    return run


# ---- comparison -----------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize])


def assert_identical(got, want, what=""):
    """same dtype and shape, NaNs in the same places (whatever their payload), every other value bit for bit"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    parts = [(got, want)] if got.dtype.kind != "c" else [(got.real, want.real), (got.imag, want.imag)]
    for g, w in parts:
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), what
        bad = (bits(g) != bits(w)) & ~nan
        assert not bad.any(), (what, int(bad.sum()), g[bad][:4], w[bad][:4])


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def specials(dtype, extremes=True):
    """+-0, +-inf, NaN and a few ordinary values of a real dtype; extremes: also the largest and the smallest normal number
    and subnormals (those of float32, and the dtype's own smallest)"""
    fi = np.finfo(dtype)
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0, 0.5, -3.25, 1e-3, 1e3]
    if extremes:
        v += [float(fi.max), float(fi.tiny), 1e-45, -1e-45, 1e-40, 7e-39, float(fi.smallest_subnormal)]
    return np.array(v, dtype=dtype)


def special_pairs(dtype, extremes=True):
    """every special value against every special value, plus random values: (x, y)"""
    s = specials(dtype, extremes)
    rng = np.random.default_rng(5)
    r = (rng.standard_normal(64) * 10.0 ** rng.integers(-3, 4, 64)).astype(dtype)
    return np.concatenate([np.repeat(s, s.size), r]), np.concatenate([np.tile(s, s.size), r[::-1]])


def moduli(n, dtype, seed, positive=False):
    """n values with moduli in [1e-3, 1e3] (log-uniform): real with random signs, or complex with random phases"""
    rng = np.random.default_rng(seed)
    m = 10.0 ** rng.uniform(-3, 3, n)
    if np.dtype(dtype).kind == "c":
        return (m * np.exp(2j * np.pi * rng.uniform(0, 1, n))).astype(dtype)
    return (m if positive else m * rng.choice([-1.0, 1.0], n)).astype(dtype)


def wider(dtype):
    return {"f4": np.float64, "c8": np.complex128, "f8": np.longdouble, "c16": np.clongdouble}[np.dtype(dtype).str[1:]]


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype).itemsize // (2 if np.dtype(dtype).kind == "c" else 1) == 4 else 2.0 ** -53


def max_relative_error(got, exact):
    """the largest |got - exact| / |exact| over the elements where exact is finite and not zero, in units of 1"""
    exact = np.asarray(exact)
    ok = np.isfinite(exact) & (exact != 0)
    return float(np.max(np.abs(got.astype(exact.dtype)[ok] - exact[ok]) / np.abs(exact[ok])))


# ---- the parity checks of the issue ------------------------------------------------------------------------------------------
def check_real_exact(apply, dtype):
    """real + - * / with both orders, against a scalar, an array and the special values: NumPy's bits"""
    x, y = special_pairs(dtype)
    with np.errstate(all="ignore"):
        for op, f in (("+", np.add), ("-", np.subtract), ("*", np.multiply), ("/", np.divide)):
            assert_identical(apply(x, y, op, False), f(x, y), (op, dtype))
            assert_identical(apply(x, y, op, True), f(y, x), ("r" + op, dtype))
        for s in (3, 2.5, -0.1, 1e-40):
            for op, f in (("+", np.add), ("-", np.subtract), ("*", np.multiply), ("/", np.divide)):
                assert_identical(apply(x, s, op, False), f(x, s), (op, s, dtype))
                assert_identical(apply(x, s, op, True), f(s, x), ("r" + op, s, dtype))
        assert_identical(apply(x, 0, "/", True), np.divide(0, x), ("0 / x", dtype))


def check_power_fast_paths(apply, dtype):
    """exponents 2, 1, 0, 0.5 and -1 as Python int or float: first that NumPy still takes its fast paths (so that a change
    there shows up as such), then NumPy's bits"""
    x = np.concatenate([specials(dtype), moduli(500, dtype, 7)])
    with np.errstate(all="ignore"):
        paths = {2: x * x, 2.0: x * x, 1: x.copy(), 1.0: x.copy(), 0: np.ones_like(x), 0.0: np.ones_like(x), 0.5: np.sqrt(x),
                 -1: 1 / x, -1.0: 1 / x}
        for e, want in paths.items():
            assert_identical(x ** e, want, ("NumPy's own fast path", e, dtype))
            assert_identical(apply(x, e, "**", False), want, ("**", e, dtype))


def check_complex(apply, dtype):
    """complex + - bit for bit; complex * within 4.5 u |x| |y| (NumPy's product is fused, error 2 u; the textbook one
    sqrt(5) u).  The special values here are +-0, +-inf and NaN: the bound models neither underflow nor overflow, and an
    overflowing product is a NaN in one formulation and an infinity in the other."""
    real = np.float32 if np.dtype(dtype) == np.complex64 else np.float64
    sx, sy = special_pairs(real, extremes=False)
    x, y = np.empty(sx.size, dtype=dtype), np.empty(sx.size, dtype=dtype)
    x.real, x.imag, y.real, y.imag = sx, sy, sy[::-1], -2 * sx
    x, y = np.concatenate([x, moduli(4000, dtype, 1)]), np.concatenate([y, moduli(4000, dtype, 2)])
    u = unit_roundoff(dtype)
    with np.errstate(all="ignore"):
        for op, f in (("+", np.add), ("-", np.subtract)):
            assert_identical(apply(x, y, op, False), f(x, y), (op, dtype))
            assert_identical(apply(x, y, op, True), f(y, x), ("r" + op, dtype))
            assert_identical(apply(x, 2 - 3j, op, False), f(x, dtype(2 - 3j)), (op, "scalar", dtype))
        want, got = x * y, apply(x, y, "*", False)
        assert got.dtype == want.dtype
        fin = np.isfinite(want.real) & np.isfinite(want.imag) & np.isfinite(x) & np.isfinite(y)
        big = np.abs(x.astype(wider(dtype))) * np.abs(y.astype(wider(dtype)))
        fin &= big < np.finfo(real).max / 4                              # (and none of overflow)
        err = np.abs(got.astype(wider(dtype)) - want.astype(wider(dtype)))
        ratio = float(np.max(err[fin] / np.maximum(big[fin], np.finfo(real).tiny))) / u
        print(f"complex * {np.dtype(dtype).name}: max |kernel - NumPy| = {ratio:.2f} u |x| |y| (bound 4.5)")
        assert ratio <= 4.5, ratio
        for part in ("real", "imag"):                                    # outside that set: NaNs where NumPy has them
            assert np.array_equal(np.isnan(getattr(got, part))[~fin], np.isnan(getattr(want, part))[~fin])


def _error_vs_numpy(got, want, exact, what):
    e_ref, e_ker = max_relative_error(want, exact), max_relative_error(got, exact)
    u = unit_roundoff(want.dtype)
    print(f"{what} {want.dtype.name}: E_ref = {e_ref / u:.2f} u, kernel = {e_ker / u:.2f} u")
    assert got.dtype == want.dtype
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert e_ker <= 2 * e_ref, (what, e_ker / u, e_ref / u)
    return e_ref / u, e_ker / u


def check_complex_division(apply, dtype):
    """complex / against the exact quotient in the next wider type: at most twice NumPy's own largest relative error"""
    x, y = moduli(10000, dtype, 3), moduli(10000, dtype, 4)
    w = wider(dtype)
    return _error_vs_numpy(apply(x, y, "/", False), x / y, x.astype(w) / y.astype(w), "complex /")


def check_power(apply, dtype):
    """real ** with exponents that have no fast path, the same way; negative bases give NaN exactly where NumPy's do"""
    w = wider(dtype)
    x = moduli(10000, dtype, 6, positive=True)
    worst = (0.0, 0.0)
    with np.errstate(all="ignore"):
        for e in (2.5, -0.3, 3, 1.0 / 3):
            ew = w(dtype(e)) if isinstance(e, float) else e                   # the exponent as NumPy rounds it
            r = _error_vs_numpy(apply(x, e, "**", False), x ** e, x.astype(w) ** ew, f"x ** {e:.3g}")
            worst = max(worst, r, key=lambda t: t[1])
        y = moduli(10000, dtype, 8) / dtype(200)                              # exponents in about [-5, 5]
        _error_vs_numpy(apply(x, y, "**", False), x ** y, x.astype(w) ** y.astype(w), "x ** array")
        neg = np.array([-2.0, -2.0, -0.5, -8.0, -1.0, -3.0, -0.0], dtype=dtype)
        ye = np.array([3.0, 0.5, 2.0, 1.0 / 3, -2.5, -3.0, -1.5], dtype=dtype)
        got, want = apply(neg, ye, "**", False), neg ** ye
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() >= 3
        assert np.allclose(got, want, rtol=4 * unit_roundoff(dtype), atol=0, equal_nan=True)
        for e in (3, 2.5):
            got, want = apply(neg, e, "**", False), neg ** e
            assert np.array_equal(np.isnan(got), np.isnan(want))
    return worst


def needs_longdouble(dtype):
    """None, or why the 64-bit cases of the error comparison cannot run here"""
    if np.dtype(dtype).str[1:] in ("f8", "c16") and np.finfo(np.longdouble).nmant < 63:
        return f"np.longdouble has {np.finfo(np.longdouble).nmant} mantissa bits: no wider type than float64 here"
    return None


# ---- shapes at the kernel's dispatch edges ---------------------------------------------------------------------------------
EDGE_SAMPLES = (1, 3, 4, 5, 257)
EDGE_CHANNELS = (1, 3, 4, 5)


def edge_analog(nchan, dtype=np.float32, seed=0, gap=1):
    """(data, trialdefinition): trials of 1, 3, 4, 5 and 257 samples with `gap` unused rows in front of each (odd starts:
    with 3 or 5 channels hardly a trial begins on a 16-byte boundary)"""
    rng = np.random.default_rng(seed)
    trl, at = [], 0
    for n in EDGE_SAMPLES:
        at += gap
        trl.append([at, at + n, -1])
        at += n
    x = rng.standard_normal((at + 2, nchan))
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(x.shape)
    return x.astype(dtype), np.array(trl, dtype=float)
