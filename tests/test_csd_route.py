"""Which kernels serve a cross-spectral update, over which ranges and in which order: the pure route of
syncopy_amd/csrc/csd_route.h, compiled with the host compiler alone (no HIP, no device) and asked through a small C shim
(tests/emu/csd_route_shim.cpp).  The library and the kernel emulator both walk the steps this header returns."""
import ctypes as C

import pytest

import build_emu

CAP = 4096


@pytest.fixture(scope="module")
def lib():
    lib = build_emu.build_shim("csd_route_shim.cpp", "libspycsdroute.so")
    lib.csd_recut_main.restype = lib.csd_tri_tiles.restype = lib.csd_route_sweep.restype = C.c_longlong
    return lib


def route(lib, nchan, nfreq, nrows, blocked=0, exact=0, num_cu=256, m3=0):
    """(err, kernel name, step lines, message).  m3: 0 every padded 3M width is built, 1 the emulator's sample, 2 none.
    The message of a route without error is the shim's verdict on its coverage (empty: every (frequency, tile, row)
    exactly once)."""
    geom = (C.c_longlong * 6)()
    name, steps, msg = (C.create_string_buffer(CAP) for _ in range(3))
    err = lib.csd_route_text(nchan, nfreq, C.c_longlong(nrows), blocked, exact, C.c_longlong(num_cu), m3, geom, name, steps, msg, CAP)
    return err, name.value.decode(), steps.value.decode().splitlines(), msg.value.decode()


# (nchan, nfreq, nrows, blocked, phase-exact, num_cu, m3), kernel name, steps in launch order
ROUTES = [
    ((256, 5, 70, 0, 0, 256, 0), 'spycsd::csd3m_kernel<256, 8, true, false, false>', [
        'M3_EXACT rows 0+70 nprow 5',
    ]),
    ((256, 259, 70, 0, 0, 256, 0), 'spycsd::csd3m_kernel<256, 8, true, false, false>', [
        'M3_EXACT rows 0+70 nprow 256',
        'TAIL rows 0+70 items 9216:9324 split 2x36 grid 14 lds 98304 kb 8',
    ]),
    ((256, 2049, 70, 0, 0, 256, 0), 'spycsd::csd3m_kernel<256, 8, true, false, false>', [
        'M3_EXACT rows 0+70 nprow 2048',
        'TAIL rows 0+70 items 73728:73764 split 2x36 grid 5 lds 98304 kb 8',
    ]),
    ((256, 2049, 70, 1, 0, 256, 0), 'spycsd::csd3m_kernel<256, 8, true, false, false>', [
        'M3_EXACT rows 0+70 nprow 2048',
        'TAIL rows 0+70 items 73728:73764 split 2x36 grid 5 lds 98304 kb 8',
    ]),
    ((256, 2049, 70, 0, 1, 256, 0), 'spycsd::csd_accum_kernel<5, 4, 1>', [
        'ACCUM<5,4,1> rows 0+70 items 0:73728 grid 2048 lds 98816 kb 16',
        'TAIL rows 0+70 items 73728:73764 split 2x36 grid 5 lds 98304 kb 8',
    ]),
    ((64, 1027, 70, 0, 0, 256, 0), 'spycsd::csd3m_kernel<64, 8, false>', [
        'M3_PADDED<64> rows 0+70 nprow 256',
        'TAIL rows 0+70 items 3072:3081 split 2x36 grid 2 lds 98304 kb 16',
    ]),
    ((255, 259, 7, 0, 0, 256, 0), 'spycsd::csd3m_kernel<256, 8, false>', [
        'M3_PADDED<256> rows 0+6 nprow 256',
        'TAIL rows 0+6 items 9216:9324 split 1x0 grid 14 lds 98304 kb 8',
        'ACCUM<5,4,2> rows 6+1 items 0:9216 grid 256 lds 98816 kb 16',
        'TAIL rows 6+1 items 9216:9324 split 1x0 grid 14 lds 49152 kb 4',
    ]),
    ((301, 259, 7, 0, 0, 256, 0), 'spycsd::csd3m_kernel<304, 8, false>', [
        'M3_PADDED<304> rows 0+6 nprow 256',
        'TAIL rows 0+6 items 14080:14245 split 1x0 grid 21 lds 61440 kb 4',
        'ACCUM<5,4,3> rows 6+1 items 0:14080 grid 512 lds 98816 kb 8',
        'ACCUM<1,1,0> rows 6+1 items 14080:14245 grid 21 lds 61440 kb 4',
    ]),
    ((300, 259, 6, 0, 0, 256, 0), 'spycsd::csd3m_kernel<304, 8, false>', [
        'M3_PADDED<304> rows 0+6 nprow 256',
        'TAIL rows 0+6 items 14080:14245 split 1x0 grid 21 lds 61440 kb 4',
    ]),
    ((300, 259, 6, 0, 0, 256, 2), 'spycsd::csd_accum_kernel<5, 4, 3>', [
        'ACCUM<5,4,3> rows 0+6 items 0:14080 grid 512 lds 98816 kb 8',
        'ACCUM<1,1,0> rows 0+6 items 14080:14245 grid 21 lds 61440 kb 4',
    ]),
    ((512, 259, 6, 0, 0, 256, 0), 'spycsd::csd3m_kernel<512, 8, false>', [
        'M3_PADDED<512> rows 0+6 nprow 256',
        'TAIL rows 0+6 items 34816:35224 split 1x0 grid 51 lds 98304 kb 4',
    ]),
    ((512, 259, 6, 0, 0, 256, 2), 'spycsd::csd_accum_kernel<5, 4, 3>', [
        'ACCUM<5,4,3> rows 0+6 items 0:34816 grid 1024 lds 98816 kb 8',
        'ACCUM<1,1,0> rows 0+6 items 34816:35224 grid 51 lds 98304 kb 4',
    ]),
    ((513, 5, 7, 0, 0, 256, 0), 'spycsd::csd3m_kernel<512, 8, false, true> (+ csd3m_kernel<256, 8, false> per 256-channel block)', [
        'M3_PADDED<256> rows 0+6 nprow 5 ch 0+256',
        'M3_PADDED<256> rows 0+6 nprow 5 ch 256+256',
        'M3_RECT rows 0+6 nfreq 5 ch 256+256 x 0+256',
        'M3_PADDED<16> rows 0+6 nprow 1 ch 512+1',
        'M3_RECT rows 0+6 nfreq 5 ch 512+1 x 0+256',
        'M3_RECT rows 0+6 nfreq 5 ch 512+1 x 256+256',
        'RANK1 rows 6+1',
    ]),
    ((640, 5, 6, 0, 0, 256, 0), 'spycsd::csd3m_kernel<512, 8, false, true> (+ csd3m_kernel<256, 8, false> per 256-channel block)', [
        'M3_PADDED<256> rows 0+6 nprow 5 ch 0+256',
        'M3_PADDED<256> rows 0+6 nprow 5 ch 256+256',
        'M3_RECT rows 0+6 nfreq 5 ch 256+256 x 0+256',
        'M3_PADDED<128> rows 0+6 nprow 3 ch 512+128',
        'M3_RECT rows 0+6 nfreq 5 ch 512+128 x 0+256',
        'M3_RECT rows 0+6 nfreq 5 ch 512+128 x 256+256',
    ]),
    ((1025, 3, 6, 0, 1, 256, 0), 'spycsd::csd3m_kernel<512, 8, false, true, true> (+ csd3m_kernel<256, 8, false, false, true> per 256-channel block)', [
        'M4_BLOCK rows 0+5 nfreq 3 ch 0+256',
        'M4_BLOCK rows 0+5 nfreq 3 ch 256+256',
        'M4_RECT rows 0+5 nfreq 3 ch 256+256 x 0+256',
        'M4_BLOCK rows 0+5 nfreq 3 ch 512+256',
        'M4_RECT rows 0+5 nfreq 3 ch 512+256 x 0+256',
        'M4_RECT rows 0+5 nfreq 3 ch 512+256 x 256+256',
        'M4_BLOCK rows 0+5 nfreq 3 ch 768+256',
        'M4_RECT rows 0+5 nfreq 3 ch 768+256 x 0+256',
        'M4_RECT rows 0+5 nfreq 3 ch 768+256 x 256+256',
        'M4_RECT rows 0+5 nfreq 3 ch 768+256 x 512+256',
        'M4_BLOCK rows 0+5 nfreq 3 ch 1024+1',
        'M4_RECT rows 0+5 nfreq 3 ch 1024+1 x 0+256',
        'M4_RECT rows 0+5 nfreq 3 ch 1024+1 x 256+256',
        'M4_RECT rows 0+5 nfreq 3 ch 1024+1 x 512+256',
        'M4_RECT rows 0+5 nfreq 3 ch 1024+1 x 768+256',
        'RANK1 rows 5+1',
    ]),
    ((5, 9, 6, 0, 0, 256, 0), 'spycsd::csd3m_kernel<16, 8, false>', [
        'M3_PADDED<16> rows 0+5 nprow 1',
        'ACCUM<5,4,2> rows 5+1 items 0:9 grid 1 lds 98816 kb 16',
    ]),
    ((5, 9, 6, 1, 0, 256, 0), 'spycsd::csd_accum_kernel<1, 1, 0>', [
        'ACCUM<1,1,0> rows 0+6 items 0:9 grid 2 lds 49152 kb 8',
    ]),
    ((40, 5, 7, 0, 0, 256, 0), 'spycsd::csd3m_kernel<48, 8, false>', [
        'M3_PADDED<48> rows 0+7 nprow 1',
    ]),
    ((40, 5, 7, 1, 0, 256, 0), 'spycsd::csd_accum_kernel<1, 1, 0>', [
        'ACCUM<1,1,0> rows 0+7 items 0:15 grid 2 lds 49152 kb 8',
    ]),
    ((70, 3, 10, 0, 0, 256, 0), 'spycsd::csd3m_kernel<80, 8, false>', [
        'M3_PADDED<80> rows 0+10 nprow 1',
    ]),
    ((70, 3, 10, 1, 0, 256, 0), 'spycsd::csd_accum_kernel<3, 2, 0>', [
        'ACCUM<3,2,0> rows 0+10 items 0:18 grid 1 lds 82944 kb 12',
    ]),
    ((256, 5, 70, 0, 0, 4, 0), 'spycsd::csd3m_kernel<256, 8, true, false, false>', [
        'M3_EXACT rows 0+70 nprow 4',
        'TAIL rows 0+70 items 144:180 split 1x0 grid 5 lds 98304 kb 8',
    ]),
    ((256, 9, 130, 0, 0, 4, 0), 'spycsd::csd3m_kernel<256, 8, true, false, false>', [
        'M3_EXACT rows 0+130 nprow 8',
        'TAIL rows 0+130 items 288:324 split 1x0 grid 5 lds 98304 kb 8',
    ]),
    ((64, 17, 12, 0, 0, 4, 0), 'spycsd::csd3m_kernel<64, 8, false>', [
        'M3_PADDED<64> rows 0+12 nprow 4',
        'TAIL rows 0+12 items 48:51 split 1x0 grid 1 lds 73728 kb 12',
    ]),
    ((32, 33, 130, 0, 0, 4, 0), 'spycsd::csd3m_kernel<32, 8, false>', [
        'M3_PADDED<32> rows 0+130 nprow 4',
        'TAIL rows 0+130 items 32:33 split 3x44 grid 1 lds 98304 kb 16',
    ]),
    ((300, 5, 6, 0, 0, 4, 0), 'spycsd::csd3m_kernel<304, 8, false>', [
        'M3_PADDED<304> rows 0+6 nprow 5',
    ]),
    ((70, 21, 10, 1, 0, 4, 0), 'spycsd::csd_accum_kernel<3, 2, 0>', [
        'ACCUM<3,2,0> rows 0+10 items 0:126 grid 7 lds 92160 kb 8',
    ]),
    ((161, 8, 130, 1, 0, 4, 0), 'spycsd::csd_accum_kernel<5, 4, 0>', [
        'ACCUM<5,4,0> rows 0+130 items 0:144 grid 4 lds 55296 kb 4',
        'TAIL rows 0+130 items 144:168 split 1x0 grid 3 lds 73728 kb 8',
    ]),
]


@pytest.mark.parametrize("query,name,steps", ROUTES, ids=["C%d_F%d_R%d_b%d_x%d_cu%d_m%d" % q for q, _, _ in ROUTES])
def test_route_table(lib, query, name, steps):
    err, got_name, got_steps, msg = route(lib, *query)
    assert (err, msg) == (0, ""), (err, msg)
    assert got_name == name
    assert got_steps == steps


def test_every_step_list_covers_the_update_once(lib):
    """nchan 1 ... 1100 x layout x arithmetic x the frequency counts around the re-cut boundary x 1 / 70 / 301 rows: the
    steps cover every (frequency, lower-triangle tile, row) exactly once, and a tail whose rows are split starts on a
    frequency boundary (the shim's check_cover).  Both chip sizes meet re-cut tails with and without a row split."""
    # (with only a sample of the 3M instances, or none, the block walk above 512 channels has no kernels: up to 512 there)
    for num_cu, m3, top in ((4, 0, 1100), (256, 0, 1100), (4, 1, 512), (256, 2, 512)):
        tails, split_tails, msg = C.c_longlong(), C.c_longlong(), C.create_string_buffer(512)
        n = lib.csd_route_sweep(C.c_longlong(num_cu), top, m3, C.byref(tails), C.byref(split_tails), msg, 512)
        assert n == top * 2 * 2 * 8 * 3, msg.value.decode()
        assert 0 < split_tails.value < tails.value


def test_recut_main_at_its_edges(lib):
    r = lambda nwg, cu: lib.csd_recut_main(C.c_longlong(nwg), C.c_longlong(cu))
    assert r(256 + 64, 256) == 256           # rem * 4 == num_cu: the partial round is re-cut
    assert r(256 + 65, 256) == 256 + 65      # one above: it stays
    assert r(256, 256) == 256 and r(512, 256) == 512      # no partial round
    assert r(255, 256) == 255 and r(3, 256) == 3          # less than one round: nothing to re-cut
    assert r(2049, 256) == 2048 and r(259, 256) == 256
    assert r(5, 4) == 4 and r(6, 4) == 6 and r(1, 4) == 1
    assert [lib.csd_tri_tiles(c) for c in (1, 32, 33, 256, 257, 512, 1025)] == [1, 1, 3, 36, 45, 136, 561]


# what the Python policy this header replaced (backend.csd_kernel_name) returned; these strings go into bench.py's JSON
NAMES = [
    (5, False, "spycsd::csd3m_kernel<16, 8, false>"),
    (5, True, "spycsd::csd_accum_kernel<1, 1, 0>"),
    (40, True, "spycsd::csd_accum_kernel<1, 1, 0>"),
    (70, True, "spycsd::csd_accum_kernel<3, 2, 0>"),
    (161, True, "spycsd::csd_accum_kernel<5, 4, 0>"),
    (192, False, "spycsd::csd3m_kernel<192, 8, false>"),
    (255, False, "spycsd::csd3m_kernel<256, 8, false>"),
    (256, False, "spycsd::csdh_kernel"),
    (256, True, "spycsd::csd3m_kernel<256, 8, true, false, false>"),
    (300, False, "spycsd::csd3m_kernel<304, 8, false>"),
    (512, False, "spycsd::csd3m_kernel<512, 8, false>"),
    (513, False, "spycsd::csd3m_kernel<512, 8, false, true> (+ csd3m_kernel<256, 8, false> per 256-channel block)"),
    (640, True, "spycsd::csd_accum_kernel<5, 4, 0>"),
    (1025, False, "spycsd::csd3m_kernel<512, 8, false, true> (+ csd3m_kernel<256, 8, false> per 256-channel block)"),
]


def kernel_name(lib, nchan, blocked, exact=False, half=True):
    buf = C.create_string_buffer(256)
    lib.csd_name(nchan, int(blocked), int(exact), int(half), buf, 256)
    return buf.value.decode()


@pytest.mark.parametrize("nchan,blocked,name", NAMES)
def test_kernel_names_are_those_of_the_python_policy(lib, nchan, blocked, name):
    assert kernel_name(lib, nchan, blocked) == name


def test_kernel_names_follow_the_arithmetic_setting(lib):
    # SPYHIP_CSD_F32 (half=False): 256 channels stay on the float32 3M kernel
    assert kernel_name(lib, 256, False, half=False) == "spycsd::csd3m_kernel<256, 8, true, false, false>"
    # phase-exact contexts run the 4-multiplication kernels (the half-precision kernel is one of them)
    assert kernel_name(lib, 256, False, exact=True) == "spycsd::csdh_kernel"
    assert kernel_name(lib, 256, False, exact=True, half=False) == "spycsd::csd_accum_kernel<5, 4, 1>"
    assert kernel_name(lib, 256, True, exact=True) == "spycsd::csd_accum_kernel<5, 4, 0>"
    assert kernel_name(lib, 64, False, exact=True) == "spycsd::csd_accum_kernel<5, 4, 2>"
    assert kernel_name(lib, 300, False, exact=True) == "spycsd::csd_accum_kernel<5, 4, 3>"
    assert kernel_name(lib, 1025, False, exact=True).startswith("spycsd::csd3m_kernel<512, 8, false, true, true> (+ ")
    assert kernel_name(lib, 70, True, exact=True) == "spycsd::csd_accum_kernel<3, 2, 0>"


def csdh(lib, nfreq, nrows, f0, nf, num_cu=256):
    out, msg = (C.c_longlong * 8)(), C.create_string_buffer(256)
    err = lib.csdh_route_c(nfreq, C.c_longlong(nrows), f0, nf, C.c_longlong(num_cu), out, msg, 256)
    return err, list(out), msg.value.decode()


def test_half_precision_entry_splits_at_the_same_point(lib):
    # f_main, h0, h1, tail steps, tail item0, nsplit, rows_per_split, grid
    assert csdh(lib, 2049, 70, 0, 2049) == (0, [2048, 0, 2048, 1, 2048 * 36, 2, 36, 5], "")
    assert csdh(lib, 2049, 70, 0, 1024) == (0, [2048, 0, 1024, 0, 0, 0, 0, 0], "")
    assert csdh(lib, 2049, 70, 1024, 1025) == (0, [2048, 1024, 2048, 1, 2048 * 36, 2, 36, 5], "")
    assert csdh(lib, 515, 1100, 512, 3) == (0, [512, 512, 512, 1, 512 * 36, 18, 64, 14], "")
    assert csdh(lib, 256 + 64, 70, 0, 320)[1][:4] == [256, 0, 256, 1]          # rem * 4 == num_cu
    assert csdh(lib, 256 + 65, 70, 0, 321)[1][:4] == [321, 0, 321, 0]          # one above: no tail
    err, out, msg = csdh(lib, 2049, 70, 2000, 48)                              # reaches the tail without ending at nfreq
    assert err == 0 and out[:4] == [2048, 2000, 2048, 0]
    err, out, msg = csdh(lib, 515, 70, 500, 14)
    assert err == -1 and "must end at nfreq = 515" in msg


def test_route_refuses_what_no_kernel_holds(lib):
    err, _, steps, msg = route(lib, 1100, 5, 6, blocked=1)           # blocked rows this wide do not fit the staging buffer
    assert err == -3 and "1100 channels do not fit the LDS staging buffer" in msg
    err, _, _, msg = route(lib, 600, 5, 6, m3=2)
    assert err == -1 and "no 3M kernel for a block of 256 channels" in msg
    assert route(lib, 0, 5, 6)[0] == -1 and route(lib, 5, 0, 6)[0] == -1
    assert route(lib, 256, 5, 0)[:3] == (0, "spycsd::csd3m_kernel<256, 8, true, false, false>", [])
