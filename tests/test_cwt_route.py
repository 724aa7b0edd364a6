"""The host decisions of the wavelet transform - taps, block engines, groups, pieces, staging rows and the ordered steps
of a call: the pure route of syncopy_amd/csrc/cwt_route.h, compiled with the host compiler alone (no HIP, no device) and
asked through a small C shim (tests/emu/cwt_route_shim.cpp).  The library walks the steps this header returns, and the
kernel emulator runs the library (tests/emu/cwt_emu.cpp)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
CAP = 1 << 16
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def lib():
    lib = build_emu.build_shim("cwt_route_shim.cpp", "libspycwtroute.so")
    lib.cwt_route_sweep.restype = C.c_longlong
    return lib


def morlet_scales(freqs, w0=6.0):
    return (w0 + np.sqrt(2 + w0 * w0)) / (4 * np.pi * np.asarray(freqs, dtype=np.float64))


def plan(lib, nsig, scales, nchan=3, output=0, detrend=0, family=0, p0=6.0, p1=0.0, tpos=None):
    """(err, group lines, message).  The message of a plan without error is the shim's verdict on its invariants."""
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    tp = None if tpos is None else np.ascontiguousarray(tpos, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    text, msg = C.create_string_buffer(CAP), C.create_string_buffer(CAP)
    err = lib.cwt_plan_text(family, C.c_double(p0), C.c_double(p1), _dp(sc), sc.size, C.c_double(1e-3), nsig, nchan, output, detrend,
                            tp, text, msg, CAP)
    return err, text.value.decode().splitlines(), msg.value.decode()


SIZES = ("chunk", "trend", "stage_bytes", "stage_long", "xt", "work64", "pairs", "sum_set")


def steps(lib, nsig, scales, nseg, accumulate, nchan=3, output=0, detrend=0, direct=1, precision64=0, num_cu=0, stage_budget=0,
          work_budget=0, family=0, p0=6.0, p1=0.0, tpos=None):
    """(err, sizes, step lines, message); budgets and num_cu 0: the library's."""
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    tp = None if tpos is None else np.ascontiguousarray(tpos, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    text, msg, z = C.create_string_buffer(CAP), C.create_string_buffer(CAP), (C.c_longlong * 8)()
    err = lib.cwt_exec_text(family, C.c_double(p0), C.c_double(p1), _dp(sc), sc.size, C.c_double(1e-3), nsig, nchan, output, detrend,
                            tp, nseg, accumulate, direct, precision64, C.c_longlong(num_cu), C.c_longlong(stage_budget),
                            C.c_longlong(work_budget), z, text, msg, CAP)
    return err, dict(zip(SIZES, z)), text.value.decode().splitlines(), msg.value.decode()


# Morlet w0 = 6, dt = 1e-3, scale = (6 + sqrt 38) / (4 pi f), constant detrending, power; 3 segments per call.
# (name, nsig, frequencies, channels, plan lines, steps of a per-segment call, steps of a trial sum)
PINNED = [('two_direct_groups_one_staged_row',
  3000,
  [8, 30, 45, 70, 95],
  3,
  ['taps 1211,323,216,139,102',
   'group 2^10 direct V 809 halo 108 nblocks 4 scales 2,3,4 cshift 215,177,158 sidx 2,3,4 compact -',
   'group 2^11 direct V 1726 halo 161 nblocks 2 scales 1 cshift 322 sidx 1 compact -',
   'group 2^13 V 6982 halo 605 nblocks 1 scales 0 cshift 1210 sidx 0 compact 0',
   'staged 0 long - lrow - sum_pairs 1 direct_ok 1'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 47x1x3',
   'cwt2d<10,8,0> seg 0+3 group 0 sidx full rows 5 -> output grid 12x1x1',
   'cwt2d<11,4,0> seg 0+3 group 1 sidx full rows 5 -> output grid 6x1x1',
   'cwt2<13,1,0> seg 0+3 group 2 sidx compact rows 1 -> stage grid 6x1x1',
   'cwt_scatter<wide> seg 0+3 sets 3 rows 1 compact grid 12x1x3'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 47x1x3',
   'cwt2<10,4,0,pairs> seg 0+3 group 0 sidx full rows 5 -> stage grid 8x1x1',
   'cwt2<11,2,0,pairs> seg 0+3 group 1 sidx full rows 5 -> stage grid 8x1x1',
   'cwt2<13,1,0,pairs> seg 0+3 group 2 sidx full rows 5 -> stage grid 6x1x1',
   'cwt_scatter<wide> seg 0+3 sets 2 rows 5 grid 12x5x1']),
 ('own_sum_set_on_pairs',
  4500,
  [24, 40, 64, 100],
  3,
  ['taps 404,243,152,97',
   'group 2^10 direct V 782 halo 121 nblocks 6 scales 1,2,3 cshift 242,196,169 sidx 1,2,3 compact -',
   'group 2^11 direct V 1645 halo 202 nblocks 3 scales 0 cshift 403 sidx 0 compact -',
   'sum group 2^12 V 3693 halo 202 nblocks 2 scales 0,1,2,3 cshift 403,323,277,250 sidx 0,1,2,3 compact -',
   'staged - long - lrow - sum_pairs 1 direct_ok 1'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 71x1x3',
   'cwt2d<10,8,0> seg 0+3 group 0 sidx full rows 4 -> output grid 18x1x1',
   'cwt2d<11,4,0> seg 0+3 group 1 sidx full rows 4 -> output grid 9x1x1'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 71x1x3',
   'cwt2<12,1,0,pairs> seg 0+3 sum group 0 sidx full rows 4 -> stage grid 12x1x1',
   'cwt_scatter<wide> seg 0+3 sets 2 rows 4 grid 18x4x1']),
 ('pieces_and_a_16384_group',
  20000,
  [0.3, 0.5, 1.5, 20],
  3,
  ['taps 32268,19361,6454,485',
   'group 2^11 direct V 1564 halo 242 nblocks 13 scales 3 cshift 484 sidx 3 compact -',
   'group 2^14 V 9931 halo 3227 nblocks 3 scales 2 cshift 6453 sidx 2 compact 2',
   'piece 0 of long scale 0 taps 0+8192 V 8193 halo -7942 nblocks 3 scales 0 cshift 8191 sidx 0 compact 0',
   'piece 1 of long scale 0 taps 8192+8192 V 8193 halo 250 nblocks 3 scales 0 cshift 8191 sidx 0 compact 0',
   'piece 2 of long scale 0 taps 16384+8192 V 8193 halo 8442 nblocks 3 scales 0 cshift 8191 sidx 0 compact 0',
   'piece 3 of long scale 0 taps 24576+7692 V 8693 halo 16134 nblocks 3 scales 0 cshift 7691 sidx 0 compact 0',
   'piece 0 of long scale 1 taps 0+8192 V 8193 halo -1489 nblocks 3 scales 1 cshift 8191 sidx 1 compact 1',
   'piece 1 of long scale 1 taps 8192+8192 V 8193 halo 6703 nblocks 3 scales 1 cshift 8191 sidx 1 compact 1',
   'piece 2 of long scale 1 taps 16384+2977 V 13408 halo 9680 nblocks 2 scales 1 cshift 2976 sidx 1 compact 1',
   'staged 0,1,2 long 0,1 lrow 0,1 sum_pairs 0 direct_ok 1'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 313x1x3',
   'cwt2d<11,4,0> seg 0+3 group 0 sidx full rows 4 -> output grid 39x1x1',
   'cwt<14,1,0> seg 0+3 group 1 sidx compact rows 3 -> stage grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 2 sidx full rows 2 -> long side grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 3 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 4 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 5 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 6 sidx full rows 2 -> long side grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 7 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 8 sidx full rows 2 -> long side add grid 18x1x1',
   'cwt_long_convert seg 0+3 lidx compact rows 3 grid 1407x1x1',
   'cwt_scatter<wide> seg 0+3 sets 3 rows 3 compact grid 79x3x3'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 313x1x3',
   'cwt2<11,2,0> seg 0+3 group 0 sidx full rows 4 -> stage grid 39x1x1',
   'cwt<14,1,0> seg 0+3 group 1 sidx full rows 4 -> stage grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 2 sidx full rows 2 -> long side grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 3 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 4 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 5 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 6 sidx full rows 2 -> long side grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 7 sidx full rows 2 -> long side add grid 27x1x1',
   'cwt<14,1,2> seg 0+3 group 8 sidx full rows 2 -> long side add grid 18x1x1',
   'cwt_long_convert seg 0+3 lidx full rows 4 grid 1407x1x1',
   'cwt_scatter<wide> seg 0+3 sets 3 rows 4 grid 79x4x1']),
 ('trial_sum_falls_back_unpaired',
  4500,
  [0.9, 1.6, 20],
  3,
  ['taps 8999,6051,485',
   'group 2^11 direct V 1564 halo 242 nblocks 3 scales 2 cshift 484 sidx 2 compact -',
   'group 2^14 V 10334 halo 3025 nblocks 1 scales 1 cshift 6050 sidx 1 compact 1',
   'piece 0 of long scale 0 taps 0+8192 V 8193 halo 3692 nblocks 1 scales 0 cshift 8191 sidx 0 compact 0',
   'piece 1 of long scale 0 taps 8192+807 V 15578 halo 4499 nblocks 1 scales 0 cshift 806 sidx 0 compact 0',
   'staged 0,1 long 0 lrow 0 sum_pairs 0 direct_ok 1'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 71x1x3',
   'cwt2d<11,4,0> seg 0+3 group 0 sidx full rows 3 -> output grid 9x1x1',
   'cwt<14,1,0> seg 0+3 group 1 sidx compact rows 2 -> stage grid 9x1x1',
   'cwt<14,1,2> seg 0+3 group 2 sidx full rows 1 -> long side grid 9x1x1',
   'cwt<14,1,2> seg 0+3 group 3 sidx full rows 1 -> long side add grid 9x1x1',
   'cwt_long_convert seg 0+3 lidx compact rows 2 grid 159x1x1',
   'cwt_scatter<wide> seg 0+3 sets 3 rows 2 compact grid 18x2x3'],
  ['cwt_mean_np seg 0+3 grid 1x3x1',
   'cwt_stage_input seg 0+3 grid 71x1x3',
   'cwt2<11,2,0> seg 0+3 group 0 sidx full rows 3 -> stage grid 9x1x1',
   'cwt<14,1,0> seg 0+3 group 1 sidx full rows 3 -> stage grid 9x1x1',
   'cwt<14,1,2> seg 0+3 group 2 sidx full rows 1 -> long side grid 9x1x1',
   'cwt<14,1,2> seg 0+3 group 3 sidx full rows 1 -> long side add grid 9x1x1',
   'cwt_long_convert seg 0+3 lidx full rows 3 grid 159x1x1',
   'cwt_scatter<wide> seg 0+3 sets 3 rows 3 grid 18x3x1']),
 ('benchmark_c4',
  16384,
  [4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 88, 92, 96, 100],
  128,
  ['taps 2421,1211,807,606,485,404,346,303,269,243,221,202,187,173,162,152,143,135,128,122,116,111,106,101,97',
   'group 2^10 direct V 782 halo 121 nblocks 21 scales 9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24 cshift '
   '242,231,221,214,207,201,196,192,188,184,181,178,176,173,171,169 sidx 9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24 compact -',
   'group 2^11 direct V 1564 halo 242 nblocks 11 scales 4,5,6,7,8 cshift 484,443,414,393,376 sidx 4,5,6,7,8 compact -',
   'group 2^12 V 3290 halo 403 nblocks 5 scales 2,3 cshift 806,705 sidx 2,3 compact 0,1',
   'group 2^13 V 5772 halo 1210 nblocks 3 scales 0,1 cshift 2420,1815 sidx 0,1 compact 2,3',
   'sum group 2^12 V 3290 halo 403 nblocks 5 scales 2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24 cshift '
   '806,705,645,604,575,554,537,524,513,503,496,489,483,478,474,470,466,463,460,458,455,453,451 sidx '
   '2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24 compact -',
   'sum group 2^13 V 5772 halo 1210 nblocks 3 scales 0,1 cshift 2420,1815 sidx 0,1 compact -',
   'staged 2,3,0,1 long - lrow - sum_pairs 1 direct_ok 1'],
  ['cwt_mean_np seg 0+3 grid 2x3x1',
   'cwt_stage_input seg 0+3 grid 256x2x3',
   'cwt2d<10,8,0> seg 0+3 group 0 sidx full rows 25 -> output grid 504x1x1',
   'cwt2d<11,4,0> seg 0+3 group 1 sidx full rows 25 -> output grid 528x1x1',
   'cwt2<12,1,0> seg 0+3 group 2 sidx compact rows 4 -> stage grid 960x1x1',
   'cwt2<13,1,0> seg 0+3 group 3 sidx compact rows 4 -> stage grid 576x1x1',
   'cwt_scatter<wide> seg 0+3 sets 3 rows 4 compact grid 64x4x3'],
  ['cwt_mean_np seg 0+3 grid 2x3x1',
   'cwt_stage_input seg 0+3 grid 256x2x3',
   'cwt2<12,1,0,pairs> seg 0+3 sum group 0 sidx full rows 25 -> stage grid 1280x1x1',
   'cwt2<13,1,0,pairs> seg 0+3 sum group 1 sidx full rows 25 -> stage grid 768x1x1',
   'cwt_scatter<wide> seg 0+3 sets 2 rows 25 grid 64x25x1'])]


@pytest.mark.parametrize("name,nsig,freqs,nchan,groups,per_segment,trial_sum", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_plans(lib, name, nsig, freqs, nchan, groups, per_segment, trial_sum):
    sc = morlet_scales(freqs)
    err, got, msg = plan(lib, nsig, sc, nchan)
    assert (err, msg) == (0, ""), (err, msg)
    assert got == groups
    for acc, want in ((0, per_segment), (2, trial_sum)):
        err, _, got, msg = steps(lib, nsig, sc, 3, acc, nchan)
        assert (err, msg) == (0, ""), (err, msg)
        assert got == want


def test_block_length_rule(lib):
    """>= 4x the taps while that stays at or below 8192 points, then >= 2x up to 16384, never below the floor; 0: pieces."""
    b = lib.cwt_block_length
    assert [b(n, 1024) for n in (1, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096, 8191, 8192)] == \
        [1024, 1024, 2048, 2048, 4096, 4096, 8192, 8192, 8192, 8192, 16384, 16384, 0]
    assert [b(n, 4096) for n in (1, 1023, 1024, 4095, 4096, 8192)] == [4096, 4096, 8192, 8192, 16384, 0]
    assert b(1211, 1024) == 8192 and b(485, 1024) == 2048 and b(8199, 1024) == 0


def test_trial_sums_choose_their_set_before_anything_is_built(lib):
    """Floor 4096 from 4096 samples on; pairs only when every group of that set is at most 2^13, otherwise the per-segment set
    unpaired - and then no sum set is described (none is built and uploaded)."""
    sc = morlet_scales([24, 40, 64, 100])
    assert steps(lib, 4095, sc, 3, 2)[1]["sum_set"] == 0 and steps(lib, 4095, sc, 3, 2)[1]["pairs"] == 1
    assert steps(lib, 4096, sc, 3, 2)[1]["sum_set"] == 1 and steps(lib, 4096, sc, 3, 2)[1]["pairs"] == 1
    err, groups, msg = plan(lib, 4500, morlet_scales([1.6, 20]))            # 6051 taps: a 16384-point group
    assert (err, msg) == (0, "") and not [g for g in groups if g.startswith("sum ")] and groups[-1].endswith("sum_pairs 0 direct_ok 1")
    z = steps(lib, 4500, morlet_scales([1.6, 20]), 3, 2)[1]
    assert (z["pairs"], z["sum_set"], z["chunk"]) == (0, 0, 3)
    # precision64 and per-segment calls never take pairs
    assert steps(lib, 4500, sc, 3, 2, precision64=1)[1]["pairs"] == 0 and steps(lib, 4500, sc, 3, 1)[1]["pairs"] == 0


def test_budgets_cut_a_call_into_chunks_and_launches(lib):
    sc = morlet_scales([8, 30])                        # 1211 taps: staged, 323: direct
    per_seg = 1 * 3 * 3000 * 4
    err, z, got, msg = steps(lib, 3000, sc, 13, 0, stage_budget=5 * per_seg + 7)
    assert (err, msg, z["chunk"], z["stage_bytes"]) == (0, "", 5, 5 * per_seg)
    assert [g for g in got if g.startswith("cwt_scatter")] == [
        "cwt_scatter<wide> seg 0+5 sets 5 rows 1 compact grid 12x1x5", "cwt_scatter<wide> seg 5+5 sets 5 rows 1 compact grid 12x1x5",
        "cwt_scatter<wide> seg 10+3 sets 3 rows 1 compact grid 12x1x3"]
    err, z, got, msg = steps(lib, 3000, sc, 13, 2, stage_budget=1)          # at least one row set: a pair of trials
    assert (err, msg, z["chunk"], z["pairs"]) == (0, "", 2, 1) and len([g for g in got if g.startswith("cwt_scatter")]) == 7
    # float64: launches of max(2 num_cu, budget / (3 L complex128)) items; L = 8192 here
    err, z, got, msg = steps(lib, 3000, sc, 2, 0, precision64=1, num_cu=1, work_budget=4 * 3 * 8192 * 16)
    assert (err, msg, z["work64"]) == (0, "", 4 * 3 * 8192)
    assert got[1:] == ["cwt64<0> seg 0+2 wg0 0 grid 4x1x1", "cwt64<0> seg 0+2 wg0 4 grid 2x1x1",
                       "cwt_scatter<wide> seg 0+2 sets 2 rows 2 grid 12x2x2"]
    assert steps(lib, 3000, sc, 2, 0, precision64=1, num_cu=8, work_budget=1)[1]["work64"] == 6 * 3 * 8192      # all 6 items


def test_errors_keep_their_codes_and_texts(lib):
    sc = morlet_scales([8, 30])
    err, _, got, msg = steps(lib, 3000, sc, 65536, 0)
    assert (err, msg, got) == (-1, "cwt_exec: more than 65535 segments per call", [])
    err, _, got, msg = steps(lib, 3000, sc, 65536, 0, detrend=-1, nchan=1)
    assert (err, msg) == (-1, "cwt_exec: grid too large") and got == []
    # 60000 segments x 2500 groups of channel pairs x 23 blocks: the steps before the one that does not fit are kept
    err, _, got, msg = steps(lib, 20000, morlet_scales([95]), 60000, 0, nchan=20000, detrend=-1, direct=0, stage_budget=1 << 62)
    assert (err, msg) == (-1, "cwt_exec: grid too large") and got == ["cwt_stage_input seg 0+60000 grid 313x313x60000"]
    err, _, msg = plan(lib, 3000, sc, tpos=np.r_[0, 0, np.arange(1, 2999)])       # slots not increasing: staging only
    assert (err, msg) == (0, "") and _[-1].endswith("direct_ok 0")


def test_every_plan_and_call_keeps_the_invariants(lib):
    """Seeded sweep over families, signal lengths 1 ... 20000, 1 ... 30 scales, channel counts, accumulate 0 / 1 / 2, direct
    on / off, both precisions and small budgets (cwt_route_shim.cpp: check_plan, check_exec): every scale in exactly one
    group or its pieces covering its taps once; V >= 1, halo + V + reach = NB, the blocks cover the signal with no empty
    last block; the staging rows a bijection of the staged scales; the chunks tile the segments; every grid within its axis
    limit; every buffer size covering what its steps index."""
    stats, msg = (C.c_longlong * 5)(), C.create_string_buffer(4096)
    n = lib.cwt_route_sweep(20261018, 400, stats, msg, 4096)
    assert n == 400 * 37, msg.value.decode()
    print("queries", n, "pieces / several groups / own sum set / chunked calls / calls on pairs", list(stats))
    assert all(v > 0 for v in stats)


# ---- the C++ tap sampling against the oracle's kernels -----------------------------------------------------------------
# (family, p0, p1) of spycwt::sample_taps and the arguments of cwt64_ref.cwt64_taps
FAMILIES = [("Morlet", (0, 6.0, 0.0), dict(w0=6.0)), ("MorletSL", (1, 3.0, 5.0), dict(sl_cycles=3.0)),
            ("Paul4", (2, 4.0, 0.0), dict(family="Paul", order=4)), ("DOG2", (3, 2.0, 0.0), dict(family="DOG", order=2)),
            ("DOG6", (3, 6.0, 0.0), dict(family="DOG", order=6))]


def route_taps(lib, fam, scale, nsig, cap=1 << 17):
    re, im, c = np.zeros(cap), np.zeros(cap), C.c_int()
    n = lib.cwt_taps(fam[0], C.c_double(fam[1]), C.c_double(fam[2]), C.c_double(scale), C.c_double(1e-3), nsig, _dp(re), _dp(im), cap,
                     C.byref(c))
    assert n <= cap
    return re[:n] + 1j * im[:n], c.value


@pytest.mark.parametrize("name,fam,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_tap_sampling_agrees_with_the_oracle(lib, name, fam, kw):
    """Three scales, a signal shorter and one longer than the kernel: the same number of taps, the same centre, and values
    equal to float64 rounding.  The bound comes from the oracle's own two evaluation orders: it samples t = arange(...) * dt
    and divides by s inside the wavelet; handing it t = (arange(...) * (dt / s)) * s instead - the same kernel with the
    argument t / s rounded differently - moves its taps by up to 2^-49.1 (Morlet), 2^-50.6 (MorletSL), 2^-50.9 (Paul 4),
    2^-51.2 (DOG 2), 2^-50.7 (DOG 6) of the largest tap at these scales.  A third way of rounding the same argument (the
    C++ forms x = (t0 + m) dt / s, and atan / pow for Paul) is held to 4x the largest of these: 2^-47 of the largest tap,
    absolutely, per tap."""
    from cwt64_ref import cwt64_taps
    scales = np.array([0.004, 0.03, 0.11]) / (3.0 if name == "MorletSL" else 1.0)
    for nsig in (90, 5000):
        ref = cwt64_taps(nsig, scales, 1e-3, **kw)
        for sc, (h, c) in zip(scales, ref):
            got, gc = route_taps(lib, fam, sc, nsig)
            assert (got.size, gc) == (h.size, c)
            err = np.abs(got - h).max() / np.abs(h).max()
            print(name, "nsig", nsig, "scale", sc, "taps", h.size, "max error / max tap = 2^%.1f" % np.log2(max(err, 1e-300)))
            assert err < 2.0 ** -47
