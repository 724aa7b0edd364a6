"""The host code of the cross-spectral stage (csd.hip, ppc.hip, ccov.hip) on the CPU (tests/csd_drive.py): what the
launchers refuse, where they return early, their LDS limits and grid caps, and the entry points no kernel case of
tests/test_emu_kernels.py goes through (tril pack / unpack, spyhip_ccov_normalize, the split entry, the kernel name)."""
import ctypes as C

import numpy as np
import pytest

import build_emu
import csd_drive as D
from oracle import spy_oracle as O
from parity import assert_parity

ptr = D.ptr


def _spec(R, F, Cn, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(R, F, Cn)) + 1j * rng.normal(size=(R, F, Cn))).astype(np.complex64)


def test_refusals_and_early_returns():
    L, c = D.lib(), D.ctx()
    spec, acc = _spec(2, 3, 5), np.zeros((3, 5, 5), np.complex64)
    out = np.zeros((3, 5, 5), np.float32)
    s, a, o = ptr(spec), ptr(acc), ptr(out)
    d = np.zeros((3, 5, 5), np.float64)
    # null pointers
    for fn in (L.spyhip_csd_accumulate, L.spyhip_csd_accumulate_blocked):
        assert [fn(None, s, 2, 3, 5, a), fn(c, None, 2, 3, 5, a), fn(c, s, 2, 3, 5, None)] == [-1] * 3
    assert [L.spyhip_csd_finalize(None, a, 3, 5, 1.0), L.spyhip_csd_finalize(c, None, 3, 5, 1.0)] == [-1, -1]
    assert [L.spyhip_csd_set_phase_exact(None, 1), L.spyhip_csd_kernel_name(c, 5, 0, None, 8),
            L.spyhip_csd_split_fallbacks(c, None)] == [-1] * 3
    for fn in (L.spyhip_coh_normalize, L.spyhip_coh_from_accumulator):
        scale = (1.0,) if fn is L.spyhip_coh_from_accumulator else ()
        assert [fn(None, a, 3, 5, *scale, 1, o), fn(c, None, 3, 5, *scale, 1, o), fn(c, a, 3, 5, *scale, 1, None)] == [-1] * 3
        assert [fn(c, a, 3, 5, *scale, -1, o), fn(c, a, 3, 5, *scale, 8, o)] == [-1, -1]       # output out of range
    for fn in (L.spyhip_csd_tril_pack, L.spyhip_csd_tril_unpack):
        assert [fn(None, a, 3, 5, o), fn(c, None, 3, 5, o), fn(c, a, 3, 5, None)] == [-1] * 3
    jack = lambda spec_=s, S=a, direct=o, sd=ptr(d), sd2=ptr(d), ntrials=2, K=1, F=3, kind=1, T=4: \
        L.spyhip_jack_coh_accumulate(c, spec_, ntrials, K, F, 5, S, direct, kind, T, sd, sd2)              # noqa: E731
    assert [jack(spec_=None), jack(S=None), jack(direct=None), jack(sd=None), jack(sd2=None)] == [-1] * 5
    assert [jack(kind=-1), jack(kind=8), jack(F=0), jack(K=0), jack(T=1)] == [-1] * 5
    assert [L.spyhip_ppc_accumulate(c, None, 2, 1, 3, 5, a), L.spyhip_ppc_accumulate(c, s, 2, 1, 3, 5, None),
            L.spyhip_ppc_accumulate_csd(c, None, 2, 75, a), L.spyhip_ppc_accumulate_csd(c, s, 2, 75, None),
            L.spyhip_ppc_finalize(c, None, 3, 5, 5, 1, 2, o), L.spyhip_ppc_finalize(c, a, 3, 5, 5, 1, 2, None)] == [-1] * 6
    # nfreq < 1
    assert [L.spyhip_csd_accumulate(c, s, 2, 0, 5, a), L.spyhip_ppc_accumulate(c, s, 2, 1, 0, 5, a),
            L.spyhip_ppc_finalize(c, a, 0, 5, 5, 1, 2, o)] == [-1] * 3
    # ppc_finalize: one trial; lower_only on a non-square accumulator (which the full form accepts)
    assert [L.spyhip_ppc_finalize(c, a, 3, 5, 5, 1, 1, o), L.spyhip_ppc_finalize(c, a, 3, 5, 3, 1, 2, o)] == [-1, -1]
    L.emu_launch_log_reset()
    assert len(D.launches()) == 0                         # (nothing above reached a launch)
    assert L.spyhip_ppc_finalize(c, a, 3, 5, 3, 0, 2, o) == 0 and len(D.launches()) == 1
    # no rows, no trials: 0, nothing launched, nothing written
    assert [L.spyhip_csd_accumulate(c, s, 0, 3, 5, a), L.spyhip_csd_accumulate_blocked(c, s, 0, 3, 5, a),
            L.spyhip_ppc_accumulate(c, s, 0, 1, 3, 5, a), L.spyhip_ppc_accumulate_csd(c, s, 0, 75, a), jack(ntrials=0)] == [0] * 5
    assert len(D.launches()) == 0 and not acc.any() and not d.any()


def test_ccov_refusals_and_transform_lengths():
    L, c = D.lib("ccov"), D.ctx("ccov")
    assert [L.spyhip_ccov_nfft(n) for n in (0, 1, 682, 683, 349525, 349526)] == [-1, 1024, 1024, 2048, 1 << 19, -1]
    acc, out = np.zeros((513, 3, 3), np.complex64), np.zeros((300, 3, 3), np.float32)
    call = lambda ctx=c, a=ptr(acc), nfft=1024, nchan=3, n=600, norm=0, o=ptr(out): \
        L.spyhip_ccov_from_accumulator(ctx, a, nfft, nchan, n, 1.0, norm, o)                                # noqa: E731
    assert call() == 0
    assert [call(ctx=None), call(a=None), call(o=None), call(nchan=0), call(n=0), call(norm=3), call(norm=-1), call(nfft=2048),
            call(n=349526, nfft=1 << 19)] == [-1] * 9
    assert [L.spyhip_ccov_normalize(None, ptr(out), 4, 3), L.spyhip_ccov_normalize(c, None, 4, 3),
            L.spyhip_ccov_normalize(c, ptr(out), 0, 3), L.spyhip_ccov_normalize(c, ptr(out), 4, 0)] == [-1] * 4
    # above 8192 points the lags go through the tapered-FFT plan, which this emulator unit refuses (ccov_emu.cpp)
    long_acc, long_out = np.zeros((8193, 1, 1), np.complex64), np.zeros((4500, 1, 1), np.float32)
    assert L.spyhip_ccov_nfft(9000) == 16384
    assert call(a=ptr(long_acc), nfft=16384, nchan=1, n=9000, o=ptr(long_out)) == D.NOT_EMULATED


@pytest.mark.parametrize("entry", ["ppc", "jack"])
def test_taper_count_at_the_lds_limit(entry):
    """1 KiB of LDS per taper (two staging buffers of two 32-channel tiles): with 16 KiB per workgroup 16 tapers run, 17 are
    refused with -3 before anything is launched."""
    L, c = D.lib(), D.ctx(lds_per_block=16 * 1024)
    F, Cn = 1, 2
    acc, d, d2 = np.zeros((F, Cn, Cn), np.complex64), np.zeros((F, Cn, Cn), np.float64), np.zeros((F, Cn, Cn), np.float64)
    S = np.ones((F, Cn, Cn), np.complex64)
    direct = np.zeros((F, Cn, Cn), np.float32)

    def run(K):
        spec = _spec(K, F, Cn, K)
        if entry == "ppc":
            return L.spyhip_ppc_accumulate(c, ptr(spec), 1, K, F, Cn, ptr(acc))
        return L.spyhip_jack_coh_accumulate(c, ptr(spec), 1, K, F, Cn, ptr(S), ptr(direct), 1, 3, ptr(d), ptr(d2))
    L.emu_launch_log_reset()
    assert run(17) == -3 and len(D.launches()) == 0 and not acc.any() and not d2.any()
    assert run(16) == 0
    assert D.launches().tolist() == [[8, 1, 1, 256, 1, 1, 16 * 1024]]
    assert (acc if entry == "ppc" else d2).any()


@pytest.mark.parametrize("F,Cn", [(3, 5), (2, 33)])
@pytest.mark.parametrize("cap", [0, 1])
def test_tril_pack_unpack(F, Cn, cap):
    """Pack, clear, unpack: the lower triangle comes back exactly and nothing else is written.  cap 1: at most four
    workgroups (4 x elementwise_blocks), so that 33 channels (9 workgroups' worth) stride."""
    L, c = D.lib(), D.ctx(elementwise_blocks=cap)
    acc = _spec(F, Cn, Cn, Cn)
    ntri = Cn * (Cn + 1) // 2
    packed = np.zeros((F, ntri), np.complex64)
    L.emu_launch_log_reset()
    assert L.spyhip_csd_tril_pack(c, ptr(acc), F, Cn, ptr(packed)) == 0
    ii, jj = np.tril_indices(Cn)
    np.testing.assert_array_equal(packed, acc[:, ii, jj])
    back = np.zeros_like(acc)
    assert L.spyhip_csd_tril_unpack(c, ptr(packed), F, Cn, ptr(back)) == 0
    np.testing.assert_array_equal(back[:, ii, jj], acc[:, ii, jj])
    iu, ju = np.triu_indices(Cn, 1)
    assert not back[:, iu, ju].any()
    nwg = -(-F * Cn * Cn // 256)
    assert D.launches()[:, 0].tolist() == [min(nwg, 4) if cap else nwg] * 2


def test_ccov_normalize_alone():
    """spyhip_ccov_normalize in place against O.normalize_ccov in float64.  Tolerance: the kernel rounds the product of
    the two variances, its square root and the quotient to float32, at most 2^-24 relative each (the root halves what it
    inherits): 2.5 x 2^-24 in all, asserted as 4 x 2^-24 of each element."""
    nlag, Cn = 4, 3
    rng = np.random.default_rng(43)
    cc = rng.normal(size=(nlag, Cn, Cn)).astype(np.float32)
    cc[0, range(Cn), range(Cn)] = np.abs(cc[0, range(Cn), range(Cn)]) + 1.0
    ref = O.normalize_ccov(cc.astype(np.float64)[:, None])[:, 0]
    L = D.lib("ccov")
    L.emu_launch_log_reset()
    assert L.spyhip_ccov_normalize(D.ctx("ccov"), ptr(cc), nlag, Cn) == 0
    assert_parity(cc.astype(np.float64), ref, rtol=4 * 2.0 ** -24, atol_rel=0.0, what="ccov_normalize")
    assert build_emu.launches(L)[:, 0].tolist() == [1, 1]             # the diagonal, then the quotient


@pytest.mark.parametrize("cap", [1, 2])
def test_coh_normalize_grid_stride(cap):
    """2 x cap workgroups walk what the library's cap gives 2 workgroups per frequency: the same bits."""
    F, Cn = 3, 21                      # 1323 elements: 6 workgroups of 256 uncapped
    acc = _spec(F, Cn, Cn, cap)
    acc = (acc + acc.conj().transpose(0, 2, 1)).astype(np.complex64)
    acc[:, range(Cn), range(Cn)] += 50
    for output in ("abs", "complex"):
        D.lib().emu_launch_log_reset()
        whole = D.coh_normalize(acc, output, elementwise_blocks=0)
        few = D.coh_normalize(acc, output, elementwise_blocks=cap)
        assert D.launches()[:, 0].tolist() == [6, 2 * cap]
        np.testing.assert_array_equal(whole, few)


@pytest.mark.parametrize("cap", [1, 3])
def test_split_tail_reduction_grid_stride(cap):
    """The (32, 33, 130) case of test_csd_recut_tail on 4 compute units: three row splits whose partial sums
    csd_reduce_parts_kernel adds on 4 workgroups; capped at 1 and 3 it strides, to the same bits."""
    Cn, F, R = 32, 33, 130
    spec = _spec(R, F, Cn, 7)
    acc, few = np.zeros((F, Cn, Cn), np.complex64), np.zeros((F, Cn, Cn), np.complex64)
    D.csd_accumulate(spec, acc, num_cu=4)
    assert D.launches()[-1].tolist() == [4, 1, 1, 256, 1, 1, 0]
    D.csd_accumulate(spec, few, num_cu=4, elementwise_blocks=cap)
    assert D.launches()[-1].tolist() == [cap, 1, 1, 256, 1, 1, 0]
    np.testing.assert_array_equal(acc, few)


def test_split_entry():
    """spyhip_csd_accumulate_split: any channel count but 256 is the float32 route; 256 channels reach the fp16 matrix-core
    kernel, which has no CPU model - the emulator unit says so and runs nothing in its place."""
    L, c = D.lib(), D.ctx()
    spec = _spec(3, 2, 64, 5)
    acc, ref = np.zeros((2, 64, 64), np.complex64), np.zeros((2, 64, 64), np.complex64)
    assert D.csd_accumulate(spec, ref) == 9
    assert L.spyhip_csd_accumulate_split(c, ptr(spec), 3, 2, 64, ptr(acc), None) == 0
    np.testing.assert_array_equal(acc, ref)
    count = C.c_int(-1)
    assert L.spyhip_csd_split_fallbacks(c, C.byref(count)) == 0 and count.value == 0
    wide = _spec(1, 1, 256, 6)
    acc256, absmax = np.zeros((1, 256, 256), np.complex64), np.full(256, 8.0, np.float32)
    L.emu_launch_log_reset()
    assert L.spyhip_csd_accumulate_split_range(c, ptr(wide), 1, 1, 256, ptr(acc256), None, 0, 1) == -1
    for am in (None, ptr(absmax)):       # the library's own range pass (csdh_absmax), then the kernel itself (csdh_run)
        assert L.spyhip_csd_accumulate_split(c, ptr(wide), 1, 1, 256, ptr(acc256), am) == D.NOT_EMULATED
    assert L.spyhip_csd_accumulate_split_range(c, ptr(wide), 1, 1, 256, ptr(acc256), ptr(absmax), 0, 1) == D.NOT_EMULATED
    assert not acc256.any() and len(D.launches()) == 0


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("nchan", [5, 64, 256, 301, 521])
def test_kernel_name_is_the_route_s(nchan, blocked):
    """spyhip_csd_kernel_name of the emulated library = csd_name of the route shim (every 3M width, 256 compute units, the
    half-precision entry in use: the library's answer unless SPYHIP_CSD_F32 is set, which no test does)"""
    shim = build_emu.build_shim("csd_route_shim.cpp", "libspycsdroute.so")
    got, want = C.create_string_buffer(256), C.create_string_buffer(256)
    assert D.lib().spyhip_csd_kernel_name(D.ctx(), nchan, int(blocked), got, 256) == 0
    assert shim.csd_name(nchan, int(blocked), 0, 1, want, 256) == 0
    assert got.value and got.value == want.value
