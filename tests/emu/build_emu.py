"""Build the CPU emulation of the HIP kernels and the host-only shims of the tests (TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
CSRC = os.path.join(ROOT, "syncopy_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
OUT = os.path.join(BUILD, "libspyemu.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def build_unit(src, out, deps, flags=(), force=False):
    """Compile `src` into the shared library `out` unless `out` is newer than `src` and every file of `deps`."""
    deps = [src] + list(deps)
    if force or not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        cxx = CLANG if os.path.exists(CLANG) else "g++"
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", *flags, "-x", "c++", src, "-o", out])
    return out


def build_shim(name, out):
    """the host-only shim tests/emu/<name> over the library's headers, warnings as errors"""
    return C.CDLL(build_unit(os.path.join(HERE, name), os.path.join(BUILD, out), sources(), flags=("-Wall", "-Werror")))


def sources():
    """what the emulator units are built from: every header and .hip file of the library, and the emulator's own headers"""
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(".h")]
    return deps + [os.path.join(HERE, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "spyhip.h")]


def build(force=False):
    return build_unit(os.path.join(HERE, "emu_kernels.cpp"), OUT, sources(), force=force)


def build_library(name):
    """tests/emu/<name>_emu.cpp: the library's own .hip files of one family on the runtime stand-in hip/hip_runtime.h"""
    return build_unit(os.path.join(HERE, name + "_emu.cpp"), os.path.join(BUILD, f"lib{name}emu.so"), sources(), flags=("-I" + HERE,))


def emulated_library(name):
    """build_library(name), loaded.  Its spyhip_* functions take the types of the public ABI (syncopy_amd._lib.SIGNATURES,
    plain data)."""
    from syncopy_amd._lib import SIGNATURES
    lib = C.CDLL(build_library(name))
    for fn, (res, args) in SIGNATURES.items():
        if hasattr(lib, fn):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    lib.emu_ctx.restype, lib.emu_ctx.argtypes = C.c_void_p, [C.c_longlong] * 4
    lib.emu_ctx_set_chip.restype, lib.emu_ctx_set_chip.argtypes = None, [C.c_void_p, C.c_int, C.c_longlong]
    lib.emu_ctx_scratch.restype, lib.emu_ctx_scratch.argtypes = C.c_void_p, [C.c_void_p]
    lib.emu_ctx_destroy.restype, lib.emu_ctx_destroy.argtypes = None, [C.c_void_p]
    lib.emu_launch_log.restype, lib.emu_launch_log.argtypes = C.c_longlong, [C.c_void_p, C.c_longlong]
    return lib


def ctx(lib, grid_yz=0, elementwise_blocks=0, workgroups=0, any64_chunk=0):
    """a context of the emulated library; a launch limit that is given replaces the library's default"""
    return C.c_void_p(lib.emu_ctx(grid_yz, elementwise_blocks, workgroups, any64_chunk))


def launches(lib, reset=True):
    """(n, 7) int64: grid x y z, block x y z and dynamic LDS bytes of the launches since the last reset"""
    n = lib.emu_launch_log(None, 0)
    rows = np.zeros((n, 7), dtype=np.int64)
    lib.emu_launch_log(rows.ctypes.data_as(C.c_void_p), n)
    if reset:
        lib.emu_launch_log_reset()
    return rows


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
