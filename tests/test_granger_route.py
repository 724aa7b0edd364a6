"""Which kernels serve the Wilson / Granger stage (K6), with which grid and LDS, and where the work arrays of
spyhip_granger lie: the pure route of syncopy_amd/csrc/granger_route.h, compiled with the host compiler alone (no HIP, no
device) and asked through a small C shim (tests/emu/granger_route_shim.cpp).  granger.hip launches by this
header, and the kernel emulator runs granger.hip (tests/emu/granger_emu.cpp).

The size classes at the 160 KiB of LDS per workgroup of the MI355X (ZB = 16, ZM = 32, ZW = 64, CHP = 32, MT = 64):

    n                       products                     inverse in the iteration           Cholesky
    < 32                    zgemm_kernel                 zinv_kernel (pivoted)              zchol_kernel
    32 ... 47               zgemm_kernel                 zinv_blocked_kernel (16-row)       zchol_kernel
    48 ... 63               zgemm_mfma_kernel<0..3>      zinv_blocked_kernel                zchol_kernel
    64 ... 127, 129 ... 160,
    193 ... 224             MFMA                         zinv_mfma_kernel (32-row blocks)   zchol_panel_kernel
    128, 161 ... 192,
    225 ... 256             MFMA                         zinv64_mfma_kernel (64-row)        zchol_panel_kernel
    257 ... 288, 321 ... 352,
    385 ... 416, 449 ... 480 MFMA                        zinv_blocked_kernel (the 32-row    zchol_kernel
                                                         kernel no longer fits LDS)
    289 ... 320, 353 ... 384,
    417 ... 448, 481 ... 512 MFMA                        zinv64_mfma_kernel                 zchol_kernel
"""
import ctypes as C

import pytest

import build_emu

KIB = 1024
LDS = [160 * KIB, 64 * KIB]
CD = 16                 # bytes of a complex128


@pytest.fixture(scope="module")
def lib():
    return build_emu.build_shim("granger_route_shim.cpp", "libspygrangerroute.so")


def _ask(fn, nout, *args):
    out, name = (C.c_longlong * nout)(), C.create_string_buffer(64)
    fn(*args, out, name, 64)
    return list(out), name.value.decode()


def inv(lib, n, lds, blocked=True, has_src=True):
    """(kernel name, threads, LDS bytes, copy src first)"""
    o, name = _ask(lib.wr_inv, 4, n, int(blocked), int(has_src), C.c_ulonglong(lds))
    return name, o[1], o[2], bool(o[3])


def chol(lib, n, lds):
    o, name = _ask(lib.wr_chol, 3, n, C.c_ulonglong(lds))
    return name, o[1], o[2]


def gemm(lib, n, batch, opB=0, same=False, badd=False, ref=False):
    o, name = _ask(lib.wr_gemm, 10, n, batch, opB, int(same), int(badd), int(ref))
    return dict(name=name, mode=o[1], grid=tuple(o[2:5]), threads=o[5], lds=o[6], nmax=o[7], tiles=o[8], tpw=o[9])


def plus(lib, L, nent, lds, num_cu=256):
    o, name = _ask(lib.wr_plus, 7, L, C.c_longlong(nent), C.c_ulonglong(lds), num_cu)
    return dict(name=name, log2l=o[1], grid=o[2], threads=o[3], lds=o[4], chunk=o[5], scratch=o[6])


def test_tile_constants(lib):
    assert [lib.wr_const(i) for i in range(7)] == [32, 64, 16, 32, 512, 64, 32]          # GT, MT, ZB, ZM, ZT, ZW, CHP


# ------------------------------------------------------------------------------------------ inverse and Cholesky
def _pad(n, b):
    return (n + b - 1) // b * b


def _in(n, *bands):
    return any(lo <= n <= hi for lo, hi in bands)


def table_inverse(n):
    """The inverse column of the table above (160 KiB)."""
    if n < 32:
        return "spywil::zinv_kernel"
    if n < 64:
        return "spywil::zinv_blocked_kernel"
    if _in(n, (64, 127), (129, 160), (193, 224)):
        return "spywil::zinv_mfma_kernel"
    if _in(n, (128, 128), (161, 192), (225, 256), (289, 320), (353, 384), (417, 448), (481, 512)):
        return "spywil::zinv64_mfma_kernel"
    assert _in(n, (257, 288), (321, 352), (385, 416), (449, 480)), n
    return "spywil::zinv_blocked_kernel"


def table_cholesky(n):
    return "spywil::zchol_panel_kernel" if 64 <= n <= 256 else "spywil::zchol_kernel"


# dynamic LDS of each kernel, from the kernels' own layouts (granger_kernels.h)
INV_LDS = {
    "spywil::zinv64_mfma_kernel": lambda n: 2 * 64 * 65 * CD,                                  # D and the R panel, 64 x 65 each
    "spywil::zinv_mfma_kernel": lambda n: (32 * (_pad(n, 32) + 1) + 32 * 33) * CD,             # row block + diagonal block
    "spywil::zinv_blocked_kernel": lambda n: (16 * _pad(n, 16) + 16 * 16) * CD,
    "spywil::zinv_kernel": lambda n: n * (2 * CD + 4),                                         # pivot row, column, permutation
}
CHOL_LDS = {
    "spywil::zchol_panel_kernel": lambda n: (n * 33 + 32 * 33) * CD,
    "spywil::zchol_kernel": lambda n: n * CD,
}


def small_lds_inverse(n, lds):
    """The same order of precedence where LDS is short: a kernel that does not fit hands over to the next."""
    if n >= 128 and _pad(n, 64) == _pad(n, 32) and INV_LDS["spywil::zinv64_mfma_kernel"](n) <= lds:
        return "spywil::zinv64_mfma_kernel"
    if n >= 64 and INV_LDS["spywil::zinv_mfma_kernel"](n) <= lds:
        return "spywil::zinv_mfma_kernel"
    if n >= 32 and INV_LDS["spywil::zinv_blocked_kernel"](n) <= lds:
        return "spywil::zinv_blocked_kernel"
    return "spywil::zinv_kernel"


@pytest.mark.parametrize("lds", LDS)
def test_inverse_and_cholesky_kernels_of_every_size(lib, lds):
    for n in range(1, 513):
        name, threads, nbytes, copy = inv(lib, n, lds)
        if lds == 160 * KIB:
            assert name == table_inverse(n), n
        assert name == small_lds_inverse(n, lds), n
        assert nbytes == INV_LDS[name](n) and nbytes <= lds, (n, name, nbytes)
        assert threads == (512 if "mfma" in name else 256)
        # the matrix-core kernels read their source themselves; the others work in place on a copy
        assert copy == ("mfma" not in name)
        assert inv(lib, n, lds, has_src=False)[3] is False
        # not blocked: the pivoted kernel whatever the size
        assert inv(lib, n, lds, blocked=False) == ("spywil::zinv_kernel", 256, n * 36, True)
        cname, cthreads, cbytes = chol(lib, n, lds)
        if lds == 160 * KIB:
            assert cname == table_cholesky(n), n
        else:       # 64 KiB hold the panel of 32 columns up to n = 92
            assert cname == ("spywil::zchol_panel_kernel" if 64 <= n <= 92 else "spywil::zchol_kernel"), n
        assert cbytes == CHOL_LDS[cname](n) and cbytes <= lds and cthreads == 256


def test_band_edges(lib):
    """31 | 32, 47 | 48, 63 | 64, 127 | 128 | 129, 160 | 161, 192 | 193, 224 | 225, 256 | 257, 288 | 289, 320 | 321"""
    lds = 160 * KIB
    P, B, M, W = ("spywil::zinv_kernel", "spywil::zinv_blocked_kernel", "spywil::zinv_mfma_kernel", "spywil::zinv64_mfma_kernel")
    edges = {31: P, 32: B, 47: B, 48: B, 63: B, 64: M, 127: M, 128: W, 129: M, 160: M, 161: W, 192: W, 193: M, 224: M,
             225: W, 256: W, 257: B, 288: B, 289: W, 320: W, 321: B}
    for n, name in edges.items():
        assert inv(lib, n, lds)[0] == name, n
    for n in edges:
        assert chol(lib, n, lds)[0] == ("spywil::zchol_panel_kernel" if 64 <= n <= 256 else "spywil::zchol_kernel"), n
        assert gemm(lib, n, 9)["name"] == ("spywil::zgemm_kernel" if n < 48 else "spywil::zgemm_mfma_kernel<0>"), n


# ------------------------------------------------------------------------------------------ products
# the argument forms of the loop (granger.hip): (opB, A == B, Badd, Ref) -> MODE of zgemm_mfma_kernel
FORMS = {
    "psi^-1 U, psi (g+ + S) unfused, psi0 (g0 + S), psi psi0^-1": ((0, False, False, False), 0),
    "psi (g+ + S) fused": ((0, False, True, False), 1),
    "error check": ((1, True, False, True), 2),
    "g + I, X X^H, psi0 psi0^T": ((1, True, False, False), 3),
}


@pytest.mark.parametrize("n", [1, 31, 47, 48, 63, 64, 65, 128, 200, 256, 257, 300, 512])
@pytest.mark.parametrize("batch", [1, 8, 9, 257, 2049])
def test_product_instance_and_grid(lib, n, batch):
    for (opB, same, badd, ref), mode in FORMS.values():
        g = gemm(lib, n, batch, opB, same, badd, ref)
        assert g["threads"] == 256 and g["lds"] == 0
        if n < 48:
            assert g["name"] == "spywil::zgemm_kernel" and g["mode"] == -1
            assert g["grid"] == ((n + 31) // 32, (n + 31) // 32, batch)
            continue
        assert g["name"] == "spywil::zgemm_mfma_kernel<%d>" % mode and g["mode"] == mode
        nt = (n + 63) // 64
        tiles = nt * (nt + 1) // 2 if mode in (2, 3) else nt * nt
        assert g["tiles"] == tiles and g["tpw"] == (4 if mode == 0 else 2)
        assert g["nmax"] == tiles          # partial maxima per matrix of the error check
        grid, gy, gz = g["grid"]
        assert (gy, gz) == (1, 1) and grid % 8 == 0
        # the kernel's block map: matrix (slot // groups) * 8 + id % 8, tiles [group * tpw, (group + 1) * tpw)
        groups = grid // (8 * ((batch + 7) // 8))
        assert groups * 8 * ((batch + 7) // 8) == grid
        assert groups * g["tpw"] >= tiles > (groups - 1) * g["tpw"]          # every tile, no idle group
        assert (grid // 8 // groups) * 8 >= batch                            # every matrix


# ------------------------------------------------------------------------------------------ plus operator
@pytest.mark.parametrize("lds", LDS)
def test_plus_route(lib, lds):
    big = lds == 160 * KIB
    for L, nent in [(34, 9), (64, 9), (256, 9), (4096, 9), (5000, 9), (6000, 9), (8192, 9), (16384, 9), (16384, 2116), (4096, 65536)]:
        p = plus(lib, L, nent, lds)
        log2 = L.bit_length() - 1
        if L in (256, 512, 1024, 2048, 4096) and (big or L < 4096):          # plus4<12> needs 68 KiB
            assert p["name"] == "spywil::plus4_kernel<%d>" % log2 and p["log2l"] == log2
            assert p["threads"] == L // 16
            assert p["lds"] == max(L + (L // 16 if (L // 16) % 16 == 0 else 0) + 1, L + 2) * CD
            assert p["grid"] % 32 == 0 and p["grid"] - 32 < (nent + 1) // 2 <= p["grid"]      # one entry pair each
        elif 2 * L * CD <= lds:
            assert p["name"] == "spywil::plus_kernel" and p["grid"] == nent and p["lds"] == 2 * L * CD
        else:
            assert p["name"] == "spywil::plus_long_kernel" and p["lds"] == 0
            assert p["chunk"] == min(nent, max(256, (1 << 30) // (2 * L * CD)))
            assert p["scratch"] == p["chunk"] * 2 * L * CD and p["grid"] == p["chunk"]
        assert p["lds"] <= lds and p["threads"] <= 256
    assert [plus(lib, L, 9, 160 * KIB)["name"].split("::")[1] for L in (34, 64, 256, 4096, 5000, 6000, 8192, 16384)] == [
        "plus_kernel", "plus_kernel", "plus4_kernel<8>", "plus4_kernel<12>", "plus_kernel", "plus_long_kernel",
        "plus_long_kernel", "plus_long_kernel"]


def test_plus_long_chunks_cover_every_entry_once(lib):
    p = plus(lib, 16384, 2116, 160 * KIB)
    assert p["name"] == "spywil::plus_long_kernel" and p["chunk"] == 2048 and p["scratch"] == 1 << 30
    launches = [(e0, min(p["chunk"], 2116 - e0)) for e0 in range(0, 2116, p["chunk"])]
    assert launches == [(0, 2048), (2048, 68)]
    seen = [e0 + b for e0, ne in launches for b in range(ne)]
    assert seen == list(range(2116))
    # a chip with more CUs than 1 GiB of scratch holds entries: at least one workgroup per CU
    assert plus(lib, 1 << 20, 5000, 160 * KIB, num_cu=256)["chunk"] == 256


# ------------------------------------------------------------------------------------------ work arrays
@pytest.mark.parametrize("n,F", [(1, 3), (3, 17), (47, 65), (48, 64), (100, 65), (256, 2049), (300, 33), (512, 9)])
def test_work_arrays_do_not_overlap(lib, n, F):
    off, size = (C.c_ulonglong * 12)(), (C.c_ulonglong * 11)()
    lib.wr_arena(n, F, off, size)
    off, size = list(off), list(size)
    total = off[11]
    spans = sorted((off[i], off[i] + size[i]) for i in range(11))
    assert spans[0][0] == 0
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, (spans, n, F)
    assert spans[-1][1] <= total
    assert all(o % 256 == 0 for o in off)
    assert size[0] == F * n * n * CD and size[10] == ((n + 63) // 64) ** 2 * F * 8


# ------------------------------------------------------------------------------------------ error check
def test_subset_check_is_on_exactly_when(lib):
    for n in (1, 16, 47, 48, 49, 64, 256, 300):
        for F in (3, 9, 33, 63, 64, 65, 129, 2049):
            for forced in (0, 1):
                out = (C.c_int * 3)()
                lib.wr_err(n, F, forced, out)
                assert bool(out[0]) == (n >= 48), (n, F)
                assert bool(out[1]) == (n >= 48 and F >= 64 and not forced), (n, F, forced)
                assert out[2] == (F + 7) // 8
