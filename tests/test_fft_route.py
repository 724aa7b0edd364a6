"""Which kernel family serves a tapered FFT: the pure route of syncopy_amd/csrc/mtmfft_route.h, compiled with the host
compiler alone (no HIP, no device) and asked through a small C shim."""
import ctypes as C

import pytest

import build_emu


OUTPUT = {"pow": 0, "abs": 1, "fourier": 2, "angle": 5}
F32 = ["QUAD", "QUAD_HALF", "DEC", "DEC_HALF", "MIXED", "BLUE", "DECLONG", "LONG", "GENERIC"]
F64 = ["DEC64", "DEC64_HALF", "DECLONG64", "ANY"]
LDS = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    return build_emu.build_shim("route_shim.cpp", "libspyroute.so")


def route32(lib, nfft, output="pow", keep=True, nchan=5, ntaper=2, force=False, lds=LDS, nsig=None):
    fam, par = C.c_int(), (C.c_longlong * 8)()
    name, msg = C.create_string_buffer(256), C.create_string_buffer(256)
    err = lib.route32(nsig or nfft, nfft, nchan, ntaper, OUTPUT[output], int(keep), C.c_longlong(lds), int(force),
                      C.byref(fam), par, name, msg, 256)
    return err, F32[fam.value], name.value.decode(), msg.value.decode(), list(par)


def route64(lib, nfft, output="pow", keep=True, force=False):
    fam, par = C.c_int(), (C.c_longlong * 3)()
    name, msg = C.create_string_buffer(256), C.create_string_buffer(256)
    err = lib.route64(nfft, OUTPUT[output], int(keep), C.c_longlong(LDS), int(force), C.byref(fam), par, name, msg, 256)
    return err, F64[fam.value], name.value.decode(), msg.value.decode(), list(par)


def table(lib, which):
    buf = (C.c_int * 64)()
    return [buf[i] for i in range(lib.route_table(which, buf, 64))]


# nfft, output, keeptapers, family, kernel name (a trailing "(" marks a prefix)
NAMES = [
    (256, "pow", True, "QUAD", "mtmfft_quad_kernel<8, 16, 0, false>"),
    (4096, "fourier", True, "QUAD", "mtmfft_quad_kernel<12, 2, 2, false>"),
    (4096, "fourier", False, "QUAD", "mtmfft_quad_kernel<12, 1, 2, true>"),
    (8192, "abs", True, "QUAD", "mtmfft_quad_kernel<13, 1, 1, false>"),
    (16384, "pow", False, "QUAD_HALF", "mtmfft_quad_kernel<13, 1, 0, true, HALF of N = 16384>"),
    (128, "pow", True, "MIXED", "mtmfft_mixed_kernel<0, false> N=128 ("),
    (360, "angle", True, "MIXED", "mtmfft_mixed_kernel<1, false> N=360 ("),
    (2000, "fourier", True, "DEC", "mtmfft_dec_kernel<N = 2000, 2, false>"),
    (5000, "pow", True, "DEC_HALF", "mtmfft_dec_kernel<HALF of N = 5000, 0, false>"),
    (10000, "pow", True, "DEC", "mtmfft_dec_kernel<N = 10000, 0, false>"),
    (10000, "pow", False, "DEC_HALF", "mtmfft_dec_kernel<HALF of N = 10000, 0, true>"),
    (1009, "pow", True, "BLUE", "mtmfft_blue_kernel<11, 2, 0, false>"),
    (4093, "pow", True, "BLUE", "mtmfft_blue_kernel<13, 1, 0, false>"),
    (4097, "pow", True, "LONG", "mtmfft_long<128 x 128, 0, false>"),
    (4116, "pow", True, "GENERIC", "mtmfft_generic_kernel<0, false>"),
    (11000, "fourier", True, "LONG", "mtmfft_long<256 x 128, 2, false>"),
    (12000, "fourier", True, "DEC_HALF", "mtmfft_dec_kernel<HALF of N = 12000, 2, false>"),
    (20480, "pow", True, "DECLONG", "declong<5 x 4096, 0, false>"),
    (24000, "fourier", True, "DECLONG", "declong<6 x 4000, 2, false>"),
    (32768, "pow", False, "DECLONG", "declong<8 x 4096, 0, true>"),
    (65536, "pow", True, "LONG", "mtmfft_long<256 x 256, 0, false>"),
]


@pytest.mark.parametrize("nfft,output,keep,family,name", NAMES, ids=[f"N{c[0]}_{c[1]}_{'keep' if c[2] else 'mean'}" for c in NAMES])
def test_float32_route(lib, nfft, output, keep, family, name):
    err, fam, got, msg, _ = route32(lib, nfft, output, keep)
    assert (err, fam) == (0, family), (err, fam, got, msg)
    if name.endswith("("):
        assert got.startswith(name), got
    else:
        assert got == name


def test_float32_route_refuses_what_no_kernel_holds(lib):
    err, fam, name, msg, par = route32(lib, 600000)
    assert err == -3 and fam == "GENERIC"
    assert "LDS" in msg and str(2 * 600000 * 8) in msg and str(LDS) in msg, msg
    err, fam, name, msg, _ = route32(lib, 8, force=True)
    assert err == -1 and "too short" in msg


def test_force_generic_overrides_every_tuned_family(lib):
    for nfft in (4096, 2000, 360, 1009, 6000, 8192):
        err, fam, name, _, _ = route32(lib, nfft, force=True)
        assert (err, fam) == (0, "GENERIC") and name == "mtmfft_generic_kernel<0, false>", (nfft, fam, name)
    # (the decimation through HBM belongs to the tuned families: the float64 twin follows)
    assert route64(lib, 24000, force=True)[1] == "ANY"
    assert route64(lib, 4096, force=True)[1] == "DEC64"


def test_route_parameters(lib):
    par = route32(lib, 4096, "fourier", True)[4]
    assert par[:2] == [12, 2]
    par = route32(lib, 1009)[4]
    assert par[:4] == [11, 2, 0, 2048]
    par = route32(lib, 24000)[4]
    assert par[2:4] == [6, 4000]
    par = route32(lib, 11000)[4]
    assert par[3:7] == [32768, 8, 7, 0]
    par = route32(lib, 65536)[4]
    assert par[3:7] == [65536, 8, 8, 1]
    # MIXED: the mixed plan's LDS need decides, so a smaller LDS moves the length on (here to Bluestein)
    assert route32(lib, 360)[1] == "MIXED" and route32(lib, 360, lds=8 * 1024)[1] == "BLUE"


def test_reference_precision_route(lib):
    assert route64(lib, 4096, "pow", False)[:3] == (0, "DEC64", "mtmfft_dec64_kernel<N = 4096, 0, true>")
    for nfft in (16384, 12000):
        assert route64(lib, nfft)[:3] == (0, "DEC64_HALF", f"mtmfft_dec64_kernel<HALF of N = {nfft}, 0, false>")
    assert route64(lib, 24000, "fourier")[:3] == (0, "DECLONG64", "declong64_kernel<6 x 4000, 2, false>")
    assert route64(lib, 24000, "fourier")[4][:2] == [6, 4000]
    assert route64(lib, 360, "angle")[:3] == (0, "ANY", "mtmfft_f64_any_kernel<1, false> N=360")
    assert route64(lib, 1009)[:3] == (0, "ANY", "mtmfft_f64_any_kernel<0, false> N=1009 (Bluestein, M = 2048)")
    assert route64(lib, 1009)[4][2] == 2048
    err, fam, _, msg, _ = route64(lib, 2 ** 20 + 1)
    assert err == -3 and "2^20" in msg
    assert route64(lib, 2 ** 20)[0] == 0 and route64(lib, 1)[0] == -3


def test_length_tables_and_families_agree(lib):
    """Every entry of the three length tables routes to its family, and no other length does."""
    dec, half, dec64 = (set(table(lib, w)) for w in range(3))
    assert len(dec) == 27 and len(half) == 6 and len(dec64) == 33
    assert not (half & dec) and not (half & dec64) and min(half) > 10240 and max(half) <= 20480
    for nfft in range(16, 21001):
        for keep in (True, False):
            err, fam, name, _, _ = route32(lib, nfft, "pow", keep)
            assert err == 0
            assert (fam in ("DEC", "DEC_HALF") and nfft <= 10240) == (nfft in dec), (nfft, fam)
            assert (fam in ("DEC_HALF", "QUAD_HALF") and nfft > 10240) == (nfft in half), (nfft, fam)
            assert (f"N = {nfft}" in name) == (nfft in dec or nfft in half), (nfft, name)
            if fam == "DEC_HALF":
                assert nfft in half or nfft == 5000 or (nfft == 10000 and not keep)
        err, fam, name, _, _ = route64(lib, nfft)
        assert err == 0
        assert (fam == "DEC64") == (nfft in dec64), (nfft, fam)
        assert (fam == "DEC64_HALF") == (nfft in half), (nfft, fam)
