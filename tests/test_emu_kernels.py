"""The HIP kernel sources, compiled unchanged for the host and run workgroup-by-workgroup on OS
threads (tests/emu/hip_emu.h), against the oracle.  This checks index arithmetic, LDS layouts,
the packed-real-FFT separation and the MFMA lane maps without a GPU; the `-m gpu` tests are the
parity tests proper."""
import numpy as np
import pytest

import csd_drive as D
import cwt_drive as CD
import emu_driver as E
import granger_drive as GD
import jack_oracle as JO
from oracle import spy_oracle as O
from parity import assert_parity, excess
from cwt64_ref import assert_cwt64, cwt64_ref as _cwt64_ref, cwt64_taps


def _forced_kernel(nfft, generic=False, long=False, no_mixed=False, mixed=False, dec=None):
    """The kernel-name prefix of the family a forcing keyword asks for (None: nothing is forced)."""
    if dec is not None:
        return f"mtmfft_dec_kernel<HALF of N = {nfft}," if dec < 0 else f"mtmfft_dec_kernel<N = {nfft},"
    return ("mtmfft_generic_kernel<" if generic else "mtmfft_long<" if long else "mtmfft_blue_kernel<" if no_mixed
            else "mtmfft_mixed_kernel<" if mixed else None)


def _fft_case(nsig, nfft, nchan, K, output, keeptapers, detrend, demean_taper=False, G=None, generic=False,
              freq_idx=None, chan_idx=None, nseg=2, seed=1, long=False, no_mixed=False, nostage=False, dec=None, mixed=False,
              kernel=None):
    """`kernel`: the prefix of the kernel name the library's route gives this shape - every un-forced case states it; a
    forced case runs, and is checked for, the family of its forcing keyword (`mixed`: the mixed-radix engine on a length
    the route gives a compile-time schedule)."""
    forced = _forced_kernel(nfft, generic, long, no_mixed, mixed, dec)
    assert (forced is None) != (kernel is None), "state the expected kernel of an un-forced case (and only of those)"
    rng = np.random.default_rng(seed)
    data = rng.normal(size=(nsig * nseg + 9, nchan)).astype("f4")
    ss = np.array([4 + i * nsig for i in range(nseg)])
    taper, topt = ("dpss", {"NW": (K + 1) / 2, "Kmax": K}) if K > 1 else ("hann", {})
    tapers = O.taper_table(taper, nsig, nfft, topt)
    out = E.fft_exec(data, ss, ss, ss + nsig, nsig, nfft, tapers, O.spec_scale(nsig, nfft), detrend, demean_taper,
                     freq_idx, output, keeptapers, chan_idx=chan_idx, G=G, force_generic=generic, force_long=long,
                     no_mixed=no_mixed, mixed_nostage=nostage, dec=dec, mixed=mixed)
    assert E.LAST_KERNEL.startswith(forced or kernel), (E.LAST_KERNEL, forced or kernel)
    freqs = np.fft.rfftfreq(nfft, 1e-3)
    foi = freqs if freq_idx is None else freqs[freq_idx]
    for b in range(nseg):
        x = data[ss[b]:ss[b] + nsig]
        if chan_idx is not None:
            x = x[:, chan_idx]
        ref, _ = O.mtmfft_cF(np.array(x), foi=foi, keeptapers=keeptapers, polyremoval=None if detrend < 0 else detrend,
                             output=output, method_kwargs=dict(samplerate=1000.0, taper=taper, taper_opt=topt,
                                                               nSamples=nfft, demean_taper=demean_taper))
        assert_parity(out[b], ref[0], what=f"segment {b}")


@pytest.mark.parametrize("log2n,G", [(8, 16), (9, 8), (10, 4), (11, 2), (12, 1), (13, 1), (14, 1)])
def test_pow2_kernel_every_length(log2n, G):
    n = 1 << log2n
    nchan = 4 * G + 1 if n <= 2048 else (5 if n == 4096 else 3)   # ragged channel count: padded quads / pairs
    # (2^14: channel pairs through the 8192-point engine)
    _fft_case(n, n, nchan, 2, "pow", False, 0, G=G, nseg=1,
              kernel="mtmfft_quad_kernel<13, 1, 0, true, HALF of N = 16384>" if log2n == 14 else f"mtmfft_quad_kernel<{log2n}, {G}, 0, true>")


def test_pow2_kernel_full_quads_fast_epilogue():
    # channel counts that are multiples of 4 with every bin kept take the straight-line store path
    _fft_case(1024, 1024, 8, 2, "pow", True, 0, kernel="mtmfft_quad_kernel<10, 4, 0, false>")
    _fft_case(512, 512, 4, 2, "fourier", True, 0, kernel="mtmfft_quad_kernel<9, 8, 2, false>")
    _fft_case(256, 256, 8, 3, "pow", False, 1, kernel="mtmfft_quad_kernel<8, 16, 0, true>")
    _fft_case(512, 512, 8, 2, "abs", True, -1, kernel="mtmfft_quad_kernel<9, 8, 1, false>")
    _fft_case(300, 512, 6, 2, "fourier", True, 0, kernel="mtmfft_quad_kernel<9, 8, 2, false>")       # even, not a multiple of 4


@pytest.mark.parametrize("C,N,B,K", [(5, 256, 2, 1), (8, 512, 2, 2), (37, 256, 2, 1)])
def test_blocked_handover_layout(C, N, B, K):
    """Channel-blocked FFT -> CSD hand-over: a pure re-ordering of the spectra, identical accumulator."""
    rng = np.random.default_rng(C)
    data = rng.normal(size=(B * N, C)).astype("f4")
    ss = np.arange(B) * N
    tapers = O.taper_table("dpss", N, N, {"NW": 2.0, "Kmax": K}) if K > 1 else O.taper_table("hann", N, N)
    F = N // 2 + 1
    std = E.fft_exec(data, ss, ss, ss + N, N, N, tapers, np.sqrt(2) / N, 0, False, None, "fourier", True)
    blk = E.fft_exec(data, ss, ss, ss + N, N, N, tapers, np.sqrt(2) / N, 0, False, None, "fourier", True, blocked=True)
    assert E.LAST_KERNEL == {256: "mtmfft_quad_kernel<8, 16, 2, false>", 512: "mtmfft_quad_kernel<9, 8, 2, false>"}[N]
    nq = (C + 3) // 4
    got = blk.transpose(0, 2, 1, 3).reshape(B * K, F, 4 * nq)      # back to (rows, F, padded channels)
    np.testing.assert_array_equal(got[:, :, :C], std.reshape(B * K, F, C))
    assert np.abs(got[:, :, C:]).max(initial=0.0) < 1e-5            # padding channels: rounding residue only
    a_std = np.zeros((F, C, C), np.complex64)
    a_blk = np.zeros((F, C, C), np.complex64)
    # the blocked hand-over is served by the 4-multiplication kernels only: compare like with like (the standard
    # layout would otherwise take the 3-multiplication kernel, whose rounding differs in the last bit)
    D.csd_accumulate(std.reshape(B * K, F, C), a_std, force_4m=True)
    D.csd_accumulate(np.ascontiguousarray(blk), a_blk, blocked=True)
    np.testing.assert_array_equal(a_std, a_blk)


def test_pow2_kernel_modes():
    _fft_case(1000, 1024, 5, 3, "fourier", True, 1, demean_taper=True, kernel="mtmfft_quad_kernel<10, 4, 2, false>")
    _fft_case(1024, 1024, 5, 3, "fourier", False, 0, kernel="mtmfft_quad_kernel<10, 4, 2, true>")
    _fft_case(700, 1024, 4, 1, "abs", True, -1, kernel="mtmfft_quad_kernel<10, 4, 1, false>")
    _fft_case(512, 512, 6, 2, "real", False, 0, freq_idx=np.array([5, 0, 256, 100]), chan_idx=[5, 5, 0, 3, 1],
              kernel="mtmfft_quad_kernel<9, 8, 1, true>")


@pytest.mark.parametrize("nsig,nfft", [(2000, 2000), (500, 1000), (360, 360), (77, 154), (101, 202), (64, 64)])
def test_generic_kernel_lengths(nsig, nfft):
    # lengths that are not powers of two: Bluestein on the packed engine (M = 256 ... 4096) ...
    _fft_case(nsig, nfft, 3, 2, "pow", False, 0, no_mixed=True)
    _fft_case(nsig, nfft, 2, 1, "fourier", True, 1, demean_taper=True, nseg=1, no_mixed=True)
    # ... and the mixed-radix / Bluestein LDS kernel that still serves nfft > 4096
    _fft_case(nsig, nfft, 3, 2, "pow", False, 0, generic=True, nseg=1)


def test_long_transform_path():
    """Bluestein with four-step transforms through HBM (the path of nfft > 4096 non-powers-of-two and of
    nfft > 16384), forced onto small lengths: M = 4096 = 64 x 64 and M = 8192 = 128 x 64."""
    _fft_case(1500, 1500, 5, 2, "pow", False, 1, demean_taper=True, long=True, nseg=1)
    _fft_case(700, 900, 4, 1, "fourier", True, 0, long=True, nseg=2)
    _fft_case(2500, 2500, 3, 1, "abs", True, -1, long=True, nseg=1, freq_idx=np.array([7, 0, 1250, 333]))


@pytest.mark.parametrize("nfft,kernel", [
    (4116, "mtmfft_generic_kernel<"),       # 2^2 x 3 x 7^3: 13-smooth, above 4096, refused by the mixed engine - stays in LDS
    (4097, "mtmfft_long<128 x 128"),        # 17 x 241 above 2048: no in-LDS Bluestein, four-step transforms of 16384 points
])
def test_route_of_awkward_lengths_above_4096(nfft, kernel):
    """Shapes on which a restatement of the route once disagreed with spyfft::fft_route (it sent every such length through
    HBM): the emulator launches what the library launches."""
    _fft_case(nfft, nfft, 2, 1, "fourier", True, 0, nseg=1, kernel=kernel)


def test_forcing_keywords_are_checked():
    with pytest.raises(ValueError):         # 1024 runs four quads per workgroup
        _fft_case(1024, 1024, 4, 1, "pow", True, 0, G=2, nseg=1, kernel="mtmfft_quad_kernel<10, 4,")
    with pytest.raises(NotImplementedError):    # the route's choice, of which the emulator holds no instance: no substitute runs
        _fft_case(800, 800, 4, 1, "pow", True, 0, nseg=1, kernel="mtmfft_dec_kernel<N = 800,")


def test_bluestein_kernel_modes():
    _fft_case(500, 500, 8, 1, "pow", True, 0, no_mixed=True)       # full quads: float4 stores
    _fft_case(500, 500, 5, 3, "abs", False, 1, no_mixed=True)
    _fft_case(300, 360, 6, 2, "fourier", False, -1, no_mixed=True)
    # (un-forced from here: 77 = 7 x 11 is not 5-smooth, and the mixed engine serves no length below 16)
    _fft_case(77, 77, 4, 2, "real", True, 0, freq_idx=np.array([3, 0, 38, 20]), chan_idx=[3, 3, 0, 1],
              kernel="mtmfft_blue_kernel<8, 16, 1, false>")
    for n in (3, 5, 7, 13):                                        # trials of a handful of samples
        _fft_case(n, n, 3, 1, "fourier", True, 0, nseg=2, kernel="mtmfft_blue_kernel<8, 16, 2, false>")
    _fft_case(3, 8, 2, 1, "pow", False, -1, nseg=1, kernel="mtmfft_blue_kernel<8, 16, 0, true>")


@pytest.mark.parametrize("nsig,nfft,sched", [
    (2000, 2000, (200, 10, 2)),      # BASELINE config 1: 10 x 10 x 10 x 2
    (500, 1000, (100, 10, 10)),      # padded: 10 x 10 x 10
    (360, 360, (45, 5, 8)),          # 5 x 3 x 3 x 8
    (3000, 3000, (334, 3, 10)),      # 3 x 10 x 10 x 10: ragged butterfly counts per thread
    (5000, 5000, (500, 5, 10)),      # 5 x 10 x 10 x 10, 512 threads, 160 KB of LDS
    (64, 64, (8, 8, 8)), (16, 16, (2, 8, 2)), (25, 30, (4, 3, 10)), (1215, 1215, (135, 5, 3)),
])
def test_mixed_radix_kernel_lengths(nsig, nfft, sched):
    """K1m, the packed engine for 5-smooth lengths, with the schedule mix_schedule (the code plan_create runs) picks.
    1000, 2000, 3000 and 5000 have compile-time schedules in the library: the route gives them to mtmfft_dec_kernel, and
    the mixed engine runs them here through its filler (`mixed`), as the library would a length without a schedule."""
    how = dict(mixed=True) if nfft in (1000, 2000, 3000, 5000) else dict(kernel="mtmfft_mixed_kernel<")
    _fft_case(nsig, nfft, 5, 2, "pow", False, 0, nseg=2, **how)
    assert E.LAST_MIXED["nfft"] == nfft
    assert (E.LAST_MIXED["th"], E.LAST_MIXED["radix0"], E.LAST_MIXED["radix_last"]) == sched
    _fft_case(nsig, nfft, 2, 1, "fourier", True, 1, demean_taper=True, nseg=1, **how)


def test_mixed_radix_kernel_modes():
    _fft_case(500, 500, 8, 1, "pow", True, 0, mixed=True)          # full quads: float4 stores (500 has a compile-time schedule)
    _fft_case(500, 500, 5, 3, "abs", False, 1, mixed=True)
    mk = "mtmfft_mixed_kernel<"
    _fft_case(300, 360, 6, 2, "fourier", False, -1, kernel=mk + "2, true> N=360 (5x3x3x8)")
    _fft_case(300, 360, 9, 2, "fourier", True, 0, demean_taper=True, nostage=True, kernel=mk)     # the re-read path on a short length
    _fft_case(250, 250, 17, 2, "pow", False, 1, nostage=True, nseg=3, kernel=mk)      # several quad groups, ragged last quad
    _fft_case(80, 80, 4, 2, "real", True, 0, freq_idx=np.array([3, 0, 40, 20]), chan_idx=[3, 3, 0, 1], kernel=mk)
    _fft_case(150, 150, 4, 3, "angle", False, -1, kernel=mk)
    _fft_case(36, 36, 4, 1, "fourier", True, 0, kernel=mk + "2, false> N=36 (3x3x4)")               # 3 x 3 x 4
    assert E.LAST_MIXED["nfft"] == 36 and E.LAST_MIXED["radix_last"] == 4


def test_generic_kernel_matches_pow2_kernel():
    _fft_case(1024, 1024, 4, 2, "pow", True, 0, generic=True)


def test_zero_extended_segments():
    rng = np.random.default_rng(2)
    nsig = nfft = 256
    data = rng.normal(size=(1000, 4)).astype("f4")
    starts = np.array([-128, 0, 872, 300])
    lo = np.array([0, 0, 100, 350])
    hi = np.array([1000, 1000, 1000, 420])
    tapers = O.taper_table("hann", nsig, nfft)
    out = E.fft_exec(data, starts, lo, hi, nsig, nfft, tapers, np.sqrt(2) / nsig, 0, False, None, "fourier", True)
    assert E.LAST_KERNEL == "mtmfft_quad_kernel<8, 16, 2, false>"
    for b in range(4):
        seg = np.zeros((nsig, 4), "f4")
        for n in range(nsig):
            r = starts[b] + n
            if lo[b] <= r < hi[b]:
                seg[n] = data[r]
        seg -= seg.mean(axis=0)
        ref = (np.fft.rfft(tapers[0][:, None] * seg, axis=0) * (np.sqrt(2) / nsig)).astype(np.complex64)
        assert_parity(out[b, 0], ref, what=f"segment {b}")


def test_fp32_fft_error_level():
    """Documents the accuracy the float32 kernel delivers: ~1e-7 of the rms bin amplitude."""
    rng = np.random.default_rng(1)
    n = 4096
    data = rng.normal(size=(n, 4)).astype("f4")
    z = np.array([0])
    out = E.fft_exec(data, z, z, z + n, n, n, np.ones((1, n)), 1.0, -1, False, None, "fourier", True)[0, 0]
    assert E.LAST_KERNEL == "mtmfft_quad_kernel<12, 2, 2, false>"       # complex spectra of every taper: two quads per workgroup
    ref = np.fft.rfft(data.astype("f8"), axis=0)
    rms = np.sqrt((np.abs(ref) ** 2).mean())
    assert np.abs(out - ref).max() / rms < 1e-6
    assert np.sqrt((np.abs(out - ref) ** 2).mean()) / rms < 3e-7


@pytest.mark.parametrize("C,F,R,tpw", [(5, 9, 6, 0), (40, 5, 7, 0), (70, 3, 10, 5), (130, 2, 4, 0), (33, 4, 5, 1),
                                       (100, 3, 5, 0), (256, 2, 4, 0), (256, 1, 37, 0), (240, 1, 6, 0),
                                       # the instruction-lean path away from 256 channels: 2 / 4 / 8 frequencies per
                                       # LDS row (incl. a last, partial group), tiles crossing into the next frequency
                                       (128, 5, 6, 0), (64, 7, 5, 0), (32, 11, 4, 0), (6, 20, 3, 0),
                                       (100, 3, 5, 3), (40, 5, 7, 1),
                                       # the wide variant (512-element rows, several workgroups per frequency)
                                       (320, 2, 5, 0), (384, 1, 9, 0), (257, 1, 3, 0),
                                       # odd channel counts on the lean path: 8-byte staging loads, odd row lengths
                                       (5, 9, 6, 5), (33, 4, 5, 3), (63, 5, 6, 0), (255, 2, 4, 0)])
def test_csd_mfma_kernel(C, F, R, tpw):
    rng = np.random.default_rng(C)
    spec = (rng.normal(size=(R, F, C)) + 1j * rng.normal(size=(R, F, C))).astype(np.complex64)
    acc = np.zeros((F, C, C), np.complex64)
    D.csd_accumulate(spec[:R // 2], acc, tpw)
    D.csd_accumulate(spec[R // 2:], acc, tpw)
    fused = {o: D.coh_from_accumulator(acc, 1.0 / R, o) for o in ("abs", "complex")}
    D.csd_finalize(acc, 1.0 / R)
    for o, got in fused.items():                       # fused K5 = finalize + normalize, bit for bit
        np.testing.assert_array_equal(got, D.coh_normalize(acc, o))
    ref = (np.einsum("rfi,rfj->fij", spec.astype(np.complex128), spec.conj().astype(np.complex128)) / R)
    assert_parity(acc, ref.astype(np.complex64), what="csd")
    assert np.array_equal(acc, acc.conj().transpose(0, 2, 1)) and np.all(acc.imag[:, range(C), range(C)] == 0)
    for output in ("abs", "pow", "complex", "imag"):
        assert_parity(D.coh_normalize(acc, output), O.normalize_csd(acc, output), what=output)


@pytest.mark.parametrize("C,F,R", [(256, 2, 7), (128, 5, 9), (64, 6, 9), (192, 2, 6), (320, 1, 6),
                                   # rows narrower than the kernel's LDS image: odd counts (last row through the
                                   # 4-multiplication kernels, 8-byte aligned copies), even non-multiples of 16
                                   (37, 9, 7), (63, 5, 9), (90, 3, 6), (255, 2, 7), (301, 1, 6), (14, 20, 5)])
def test_csd_3m_kernel(C, F, R):
    """csd3m_kernel (3-multiplication complex product, 16 x 16 sub-tiles, one workgroup per frequency, rows global ->
    LDS by DMA): all 136 sub-tiles land where they belong, ragged last chunks are zero-filled, the accumulation
    continues across launches, and the result agrees with the 4-multiplication kernel to rounding.  The spectra
    carry a 40 dB spread over channels and a strong common component (coherent channels, small imaginary parts) -
    the dynamic range the 3M form is sensitive to.  128 channels: two frequencies per workgroup (72 sub-tiles), the
    odd last frequency alone in its packed row."""
    code = {256: 8}.get(C, 9)
    rng = np.random.default_rng(R)
    gain = 10 ** rng.uniform(-1, 1, size=C)
    common = rng.normal(size=(R, F, 1)) + 1j * rng.normal(size=(R, F, 1))
    spec = ((rng.normal(size=(R, F, C)) + 1j * rng.normal(size=(R, F, C)) + 2.0 * common) * gain).astype(np.complex64)
    acc = np.zeros((F, C, C), np.complex64)
    assert D.csd_accumulate(spec[:R // 2], acc) == code and D.csd_accumulate(spec[R // 2:], acc) == code
    acc4 = np.zeros((F, C, C), np.complex64)
    assert D.csd_accumulate(spec, acc4, force_4m=True) != code
    ref = np.einsum("rfi,rfj->fij", spec.astype(np.complex128), spec.conj().astype(np.complex128))
    ii, jj = np.tril_indices(C)
    # element-wise against the exact product: the error scale of an entry is sqrt(S_ii S_jj), not the global maximum
    scale = np.sqrt(np.abs(ref[:, ii, ii]) * np.abs(ref[:, jj, jj]))
    for got in (acc, acc4):
        err = np.abs(got[:, ii, jj] - ref[:, ii, jj]) / scale
        assert err.max() < 3e-6, err.max()
    assert_parity(acc[:, ii, jj], ref[:, ii, jj].astype(np.complex64), what="3M csd, lower triangle")
    D.csd_finalize(acc, 1.0 / R)
    assert np.array_equal(acc, acc.conj().transpose(0, 2, 1)) and np.all(acc.imag[:, range(C), range(C)] == 0)
    assert_parity(acc, (ref / R).astype(np.complex64), what="3M csd finalised")


@pytest.mark.parametrize("C,F,R,force_4m,code", [
    # a chip of 4 compute units: 5 packed rows (3M) / 5 workgroups (4M) leave one beyond the full round, which is re-cut.
    # 12 rows: fewer than the 128 a row split needs - the tail adds straight into the accumulator
    (64, 17, 12, False, 9), (64, 17, 12, True, 6),
    # 130 rows: the tail's rows go to 3 splits of 44, partial sums + csd_reduce_parts_kernel
    (32, 33, 130, False, 9), (32, 33, 130, True, 6)])
def test_csd_recut_tail(C, F, R, force_4m, code):
    """The workgroups beyond the last full round of the chip, re-cut into 1-tile-per-wave workgroups (csd_route.h:
    recut_main, tail_split; the steps tests/test_csd_route.py lists for these shapes), without and with the row split."""
    rng = np.random.default_rng(C + R)
    spec = (rng.normal(size=(R, F, C)) + 1j * rng.normal(size=(R, F, C))).astype(np.complex64)
    acc = np.zeros((F, C, C), np.complex64)
    assert D.csd_accumulate(spec, acc, force_4m=force_4m, num_cu=4) == code
    log = D.launches()            # the main launch, then the tail: one launch, or its rows over blockIdx.y + the reduction
    assert [tuple(r[[1, 3]]) for r in log[1:]] == ([(3, 512), (1, 256)] if R == 130 else [(1, 512)])
    whole = np.zeros((F, C, C), np.complex64)
    D.csd_accumulate(spec, whole, force_4m=force_4m)              # no tail: the last frequencies in the main launch
    ref = np.einsum("rfi,rfj->fij", spec.astype(np.complex128), spec.conj().astype(np.complex128))
    ii, jj = np.tril_indices(C)
    assert_parity(acc[:, ii, jj], ref[:, ii, jj].astype(np.complex64), what="csd with a re-cut tail, lower triangle")
    assert_parity(whole[:, ii, jj], ref[:, ii, jj].astype(np.complex64), what="csd in one launch, lower triangle")
    np.testing.assert_array_equal(acc[:-1], whole[:-1])          # the frequencies of the main launch: the same kernel


@pytest.mark.parametrize("C,F,T,K", [(5, 4, 6, 3), (40, 2, 7, 1), (70, 1, 5, 7)] + JO.PPC_EDGE_CASES)
def test_ppc_kernel(C, F, T, K):
    """K7's kernel source on the CPU: phasor sums + closed form = the oracle's walk over all trial pairs.  The shapes
    of jack_oracle.PPC_EDGE_CASES: more than 16 tapers (the generic staging walk), tile edges, four tile rows,
    frequencies around the 8-XCD mapping, a first launch of one trial."""
    rng = np.random.default_rng(C)
    spec = (rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))).astype(np.complex64)
    spec += (2.0 * rng.normal(size=(1, K, F, C))).astype(np.complex64)
    spec[..., C - 1] = 0                                # np.angle(0) = 0: consistent with everything
    st = O.spectral_dyadic_product(spec)
    ref = O.ppc(st)[0]
    first = 1 if (C, F, T, K) in JO.PPC_EDGE_CASES else 2
    U = np.zeros((F, C, C), np.complex64)
    D.ppc_accumulate(spec[:first].reshape(-1, F, C), K, U)
    D.ppc_accumulate(spec[first:].reshape(-1, F, C), K, U)
    got = D.ppc_finalize(U, T, True)
    print(f"ppc {C}-{F}-{T}-{K}: err/tol {excess(got, ref, rtol=1e-4, atol_rel=2e-5):.3f}")
    assert_parity(got, ref, what="ppc", rtol=1e-4, atol_rel=2e-5)
    assert np.array_equal(got, got.transpose(0, 2, 1)) and np.allclose(got[:, C - 1], 1, atol=1e-6)
    U2 = np.zeros((F, C, C), np.complex64)
    D.ppc_accumulate_csd(st, U2)
    assert_parity(D.ppc_finalize(U2, T, False), ref, what="ppc from csd", rtol=1e-4, atol_rel=2e-5)


@pytest.mark.parametrize("C,F,T,K,output", [(5, 3, 6, 3, "abs"), (40, 2, 5, 2, "complex"), (33, 1, 4, 1, "imag")])
def test_jackknife_coherence_kernel(C, F, T, K, output):
    """K9's kernel source on the CPU: sums of (leave-one-out coherence - direct) and of its squared modulus against a
    NumPy walk over the replicates (statistics/jackknifing.py:14-108 + csd.py:118-172)."""
    rng = np.random.default_rng(C)
    spec = (rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))).astype(np.complex64)
    spec += (1.5 * rng.normal(size=(1, K, F, C))).astype(np.complex64)
    st = O.spectral_dyadic_product(spec).astype(np.complex128)                  # (T, F, C, C)
    S = st.mean(axis=0)
    direct = O.normalize_csd(S.astype(np.complex64)[None], output)[0]
    sum_d = np.zeros((F, C, C), np.complex128 if output == "complex" else np.float64)
    sum_d2 = np.zeros((F, C, C), np.float64)
    D.jack_coh_accumulate(spec[:2].reshape(-1, F, C), K, S, direct, output, T, sum_d, sum_d2)
    D.jack_coh_accumulate(spec[2:].reshape(-1, F, C), K, S, direct, output, T, sum_d, sum_d2)
    rd, rd2 = np.zeros_like(sum_d), np.zeros_like(sum_d2)
    for t in range(T):
        loo = ((T * S - st[t]) / (T - 1)).astype(np.complex64)
        d = O.normalize_csd(loo[None], output)[0].astype(sum_d.dtype) - direct
        rd += d
        rd2 += np.abs(d) ** 2
    np.testing.assert_allclose(sum_d, rd, rtol=1e-3, atol=2e-6 * T)
    np.testing.assert_allclose(sum_d2, rd2, rtol=2e-3, atol=1e-9)


@pytest.mark.parametrize("case", JO.JACK_CASES, ids=JO.case_id)
def test_jackknife_coherence_kernel_dispatch_edges(case):
    """K9's kernel source at its dispatch edges against the float64 model and rounding bound of jack_oracle.py: both
    staging paths (16 | 17 tapers), frequency counts around the 8-XCD mapping, one to five tile rows, launches of one
    trial, every output kind; the sums continue across launches, the mirrored store is exact."""
    C, F, T, K, kind, split = case
    spec, S, direct, m = JO.case_data(case)
    sum_d = np.zeros((F, C, C), np.complex128 if kind == "complex" else np.float64)
    sum_d2 = np.zeros((F, C, C), np.float64)
    t0 = 0
    for n in split:
        D.jack_coh_accumulate(spec[t0:t0 + n].reshape(-1, F, C), K, S, direct, kind, T, sum_d, sum_d2)
        t0 += n
    assert t0 == T
    JO.check(sum_d, sum_d2, m, kind, "K9 emulated " + JO.case_id(case))


@pytest.mark.parametrize("C,N,norm", [(5, 600, 0), (6, 301, 1), (3, 1400, 2)])
def test_ccov_kernel(C, N, norm):
    """K8's kernel source on the CPU: lags from accumulated cross spectra of zero-padded trials = the oracle's
    per-pair fftconvolve walk (even N: the upper triangle one lag late, as in the reference)."""
    rng = np.random.default_rng(N)
    T = 1 if norm == 2 else 3
    x = rng.normal(size=(T, N, C))
    x[:, 2:, 1] += 0.7 * x[:, :-2, 0]
    x = (x - x.mean(axis=1, keepdims=True)).astype(np.float32)
    nlag = N // 2 + (N & 1)
    L = 1024
    while L < N + nlag:
        L *= 2
    X = np.fft.rfft(x.astype(np.float64), n=L, axis=1).astype(np.complex64)          # (T, F, C)
    acc = np.einsum("tfa,tfb->fab", X, X.conj()).astype(np.complex64)
    got = D.ccov_from_accumulator(acc, N, 1.0 / T, norm)
    ref = np.mean([O.cross_covariance(t, 1.0, None, norm == 2)[0] for t in x], axis=0)
    if norm == 1:
        ref = O.normalize_ccov(ref)
    assert_parity(got, ref[:, 0].astype(np.float32), what=f"ccov norm={norm}", atol_rel=1e-5)


@pytest.mark.parametrize("nsig,scales,detrend,output", [
    (700, [0.05, 0.02, 0.004], 0, "pow"),            # kernels of 500/200/40 taps, one block
    (3000, [0.03, 0.006], 1, "fourier"),             # several overlap-save blocks
    (300, [0.2, 0.03, 0.01], -1, "abs"),             # kernel (2000 taps) much longer than the signal: trimmed
])
def test_cwt_kernel(nsig, scales, detrend, output):
    """The staged kernels (a plan with set_direct(False)) on the blocks the plan's rule gives these scales: 2048 + 1024,
    2048 + 1024, 4096 + 2048 + 1024 points."""
    rng = np.random.default_rng(nsig)
    nchan = 3
    data = rng.normal(size=(nsig + 40, nchan)).astype("f4") + 0.5
    pre0 = 7                                          # pre-selection starts inside the trial
    ss, lo, hi = np.array([pre0 + 5]), np.array([5]), np.array([5 + nsig + 20])
    scales = np.asarray(scales)
    out = CD.cwt_exec(data, ss, lo, hi, nsig, scales, 1e-3, 6.0, detrend, output, direct=False)[0]
    trial = O.detrend(np.array(data[5:5 + nsig + 20]), None if detrend < 0 else detrend)
    ref = O.convert_output(O.cwt(trial[pre0:pre0 + nsig], 1000.0, scales).transpose(1, 0, 2), output)
    assert_parity(out, ref, what="cwt")


@pytest.mark.parametrize("output", ["pow", "fourier"])
@pytest.mark.parametrize("nbmin,nchan", [(1024, 3), (2048, 4)])
def test_cwt_direct_kernels(output, nbmin, nchan):
    """cwt2d_kernel (round 6): the transform kernel writes the (time, scale, channel) layout itself - 1024- and 2048-point
    blocks, an odd channel count (padded pair, scalar stores), plain and accumulating (out[b] += segment b) calls, a
    post-selection of samples, the channel-major input copy in front of it.  `nbmin`: the block length the plan's rule
    gives both scales (2048 points: 256 to 511 taps)."""
    rng = np.random.default_rng(nbmin + nchan)
    nsig, T = 1400, 2
    data = rng.normal(size=(T * nsig + 30, nchan)).astype("f4") + 1.5
    ss = np.array([10, nsig + 20])
    lo, hi = ss.copy(), ss + nsig
    scales = np.array({1024: [0.012, 0.004], 2048: [0.04, 0.027]}[nbmin])
    ref = np.stack([O.convert_output(O.cwt(O.detrend(np.array(data[a:a + nsig]), 0), 1000.0, scales).transpose(1, 0, 2), output)
                    for a in ss])
    trace = []
    out = CD.cwt_exec(data, ss, lo, hi, nsig, scales, 1e-3, 6.0, 0, output, trace=trace)
    assert [t.split()[0] for t in trace] == ["cwt_mean_np", "cwt_stage_input", "cwt2d<%d,%d,%d>" % (
        {1024: 10, 2048: 11}[nbmin], {1024: 8, 2048: 4}[nbmin], 2 if output == "fourier" else 0)]
    assert_parity(out, ref, what="direct cwt")
    keep = np.r_[0:3, 5:1300:9, 1023, 1024, 1399]
    tpos = np.full(nsig, -1, dtype=np.int32)
    tpos[keep] = np.arange(keep.size)
    sel = CD.cwt_exec(data, ss, lo, hi, nsig, scales, 1e-3, 6.0, 0, output, tpos=tpos, ntime_out=keep.size)
    assert_parity(sel, ref[:, keep], what="direct cwt, selected samples")


@pytest.mark.parametrize("output", ["pow", "fourier"])
@pytest.mark.parametrize("T", [4, 5])
def test_cwt_trial_sums_on_pairs_of_trials(output, T):
    """cwt2_kernel<..., PAIRT> (round 6): one channel of TWO consecutive trials in the packed halves, their sum staged;
    an odd trial count leaves the last pair half empty; 1024-point blocks, and a plan with a 2048-point group next to one."""
    rng = np.random.default_rng(T)
    nsig, nchan = 900, 3
    data = rng.normal(size=(T * nsig, nchan)).astype("f4") - 0.7
    ss = np.arange(T) * nsig
    outk = 2 if output == "fourier" else 0
    for scales, kernels in (([0.015, 0.005], ["cwt2<10,4,%d,pairs>" % outk]),
                            ([0.03, 0.015, 0.005], ["cwt2<10,4,%d,pairs>" % outk, "cwt2<11,2,%d,pairs>" % outk])):
        scales = np.array(scales)
        ref = sum(O.convert_output(O.cwt(O.detrend(np.array(data[a:a + nsig]), 0), 1000.0, scales).transpose(1, 0, 2).astype(np.complex128), output)
                  for a in ss)[None]
        trace = []
        out = CD.cwt_exec(data, ss, ss, ss + nsig, nsig, scales, 1e-3, 6.0, 0, output, accumulate=2, trace=trace)
        assert [t.split()[0] for t in trace if t.startswith("cwt2")] == kernels
        assert_parity(out, ref.astype(out.dtype), what=f"pair sums, {len(kernels)} groups")


# ---- whole plans through the route of cwt_route.h: several groups, pieces, the sum sets, chunks -----------------------------
def _cwt_plan_case(nsig, freqs_or_scales, nseg, output, accumulate=0, nchan=3, seed=0, **kw):
    """(emulated output, oracle reference, step lines) of a plan with constant detrending on `nseg` trials of nsig samples."""
    rng = np.random.default_rng(seed + nsig)
    data = rng.normal(size=(nseg * nsig + 20, nchan)).astype("f4") + 0.8
    ss = np.arange(nseg) * nsig + 10
    scales = np.asarray(freqs_or_scales, dtype=np.float64)
    ref = np.stack([O.convert_output(O.cwt(O.detrend(np.array(data[a:a + nsig]), 0), 1000.0, scales).transpose(1, 0, 2), output)
                    for a in ss])
    if accumulate == 2:
        ref = ref.astype(np.complex128 if output == "fourier" else np.float64).sum(axis=0, keepdims=True)
    trace = []
    out = CD.cwt_exec(data, ss, ss, ss + nsig, nsig, scales, 1e-3, 6.0, 0, output, accumulate=accumulate, trace=trace, **kw)
    return out, ref.astype(out.dtype), trace


def _kernels(trace):
    return [t.split()[0] for t in trace if t.startswith(("cwt<", "cwt2<", "cwt2d<", "cwt_long", "cwt_scatter"))]


def _morlet_scales(freqs):
    return (6 + np.sqrt(38)) / (4 * np.pi * np.asarray(freqs, dtype=np.float64))


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_cwt_plan_with_three_groups(output):
    """1024- and 2048-point direct groups next to a staged 4096-point group: the compact staging rows (sidx_stage, smap,
    nscales_out) run beside the direct kernels.  120, 400 and 800 taps."""
    out, ref, trace = _cwt_plan_case(1400, [0.012, 0.08, 0.04], 2, output)
    k = 2 if output == "fourier" else 0
    assert _kernels(trace) == ["cwt2d<10,8,%d>" % k, "cwt2d<11,4,%d>" % k, "cwt2<12,1,%d>" % k,
                               "cwt_scatter<%s>" % ("float2" if k else "wide")]
    assert "sidx compact rows 1 -> stage" in trace[4] and "rows 1 compact" in trace[5]
    assert_parity(out, ref, what="three groups")


@pytest.mark.parametrize("output", ["pow", "fourier"])
@pytest.mark.parametrize("accumulate,nseg", [(0, 1), (2, 3)])
def test_cwt_plan_with_a_kernel_longer_than_a_block(output, accumulate, nseg):
    """0.9 Hz on 4100 samples: 8199 taps after trimming, pieces of 8192 + 7 - the adding piece, the complex side buffer and
    its conversion (real outputs), the scale's own staging rows (complex ones).  As a trial sum of 3 trials the plan falls
    back from pairs of trials (the 16384-point kernel is not packed) to the per-segment groups."""
    out, ref, trace = _cwt_plan_case(4100, _morlet_scales([0.9, 20]), nseg, output, accumulate, nchan=2)
    k = 2 if output == "fourier" else 0
    want = ["cwt2d<11,4,%d>" % k if accumulate == 0 else "cwt2<11,2,%d>" % k, "cwt<14,1,2>", "cwt<14,1,2>"]
    want += (["cwt_long_convert"] if k == 0 else []) + ["cwt_scatter<%s>" % ("float2" if k else "wide")]
    assert _kernels(trace) == want
    assert [" add " in t for t in trace if t.startswith("cwt<14")] == [False, True]
    assert_parity(out, ref, what=f"pieces, accumulate {accumulate}")


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_cwt_trial_sums_of_long_signals_take_their_own_groups(output):
    """4100 samples, 20 and 70 Hz (485 and 139 taps: 2048- and 1024-point direct blocks per segment) as a sum of 3 trials:
    both scales on a 4096-point group of the sum set, on pairs of trials, the last pair half empty."""
    out, ref, trace = _cwt_plan_case(4100, _morlet_scales([20, 70]), 3, output, 2, nchan=2)
    k = 2 if output == "fourier" else 0
    assert _kernels(trace) == ["cwt2<12,1,%d,pairs>" % k, "cwt_scatter<%s>" % ("float2" if k else "wide")]
    assert "sum group 0" in trace[2] and "sets 2 rows 2" in trace[3]
    assert_parity(out, ref, what="own sum groups")


def test_cwt_float32_plan_in_chunks():
    """A staging budget of 5 segments: 13 segments run as chunks of 5, 5 and 3 (seg0 > 0: the segment tables, the trend and
    the output rows move with the chunk)."""
    nsig, nchan, scales = 300, 2, [0.02, 0.004]
    out, ref, trace = _cwt_plan_case(nsig, scales, 13, "abs", direct=False, nchan=nchan,
                                     stage_budget=5 * len(scales) * nchan * nsig * 4 + 100)
    assert [t.split()[2] for t in trace if t.startswith("cwt_scatter")] == ["0+5", "5+5", "10+3"]
    assert_parity(out, ref, what="three chunks")


# ---- K3 at reference precision (cwt64_kernel.h) and the direct kernels' slot bound ------------------------------------
def _cwt64_data(seed, rows, ncol, offset=0.5):
    rng = np.random.default_rng(seed)
    t = np.arange(rows)[:, None] / 1000.0
    return (rng.normal(size=(rows, ncol)) + offset + 3.0 * np.sin(2 * np.pi * 40.0 * t + np.arange(ncol))).astype("f4")


@pytest.mark.parametrize("output", ["pow", "abs", "real", "imag", "fourier"])
@pytest.mark.parametrize("detrend", [-1, 0, 1])
def test_cwt64_kernel_outputs_and_detrending(output, detrend):
    """Every output kind of cwt64_kernel and every detrending; the pre-selection starts inside the trial (seg_start !=
    trial_lo) and the trial runs past it; 13 samples: a ragged transposition tile (nsig % 4 != 0)."""
    nsig, nchan = 213, 3
    data = _cwt64_data(5 + detrend, nsig + 60, nchan)
    ss, lo, hi = np.array([17, 9]), np.array([5, 0]), np.array([5 + nsig + 40, nsig + 30])
    scales = np.array([0.04, 0.012, 0.003])
    got = CD.cwt64_exec(data, ss, lo, hi, nsig, scales, 1e-3, detrend=detrend, output=output)
    ref = _cwt64_ref(data, ss, lo, hi, nsig, scales, detrend, output)
    if detrend == 1:
        # the line fit is float64 here and float32 lstsq in the reference (VERDICT "What's missing", item 4)
        assert_parity(got, ref, what=f"cwt64 {output} detrend 1")
    else:
        assert_cwt64(got, ref, output, f"cwt64 {output} detrend {detrend}")


@pytest.mark.parametrize("family,order,sl_cycles", [("Paul", 4, None), ("DOG", 2, None), ("DOG", 6, None),
                                                    (None, None, 3.0)])
def test_cwt64_kernel_families(family, order, sl_cycles):
    """Paul, DOG (m = 2: Ricker) and MorletSL taps through the same kernel; odd channel count, a chan_idx with a repeat."""
    nsig = 301
    data = _cwt64_data(11, nsig + 10, 6)
    ci = np.array([4, 1, 4, 0, 5], dtype=np.int32)
    ss, lo, hi = np.array([3]), np.array([0]), np.array([nsig + 10])
    scales = np.array([0.02, 0.006]) if sl_cycles is None else np.array([0.004, 0.0015])
    for output in ("fourier", "abs"):
        got = CD.cwt64_exec(data, ss, lo, hi, nsig, scales, 1e-3, family=family, order=order, sl_cycles=sl_cycles,
                           detrend=0, output=output, chan_idx=ci)
        ref = _cwt64_ref(data, ss, lo, hi, nsig, scales, 0, output, chan_idx=ci, family=family, order=order,
                         sl_cycles=sl_cycles)
        assert_cwt64(got, ref, output, f"cwt64 {family or 'MorletSL'} {output}")


def test_cwt64_kernel_lengths():
    """Transform lengths at their edges: the shortest (L = 16: 5 samples, 10 taps), kernels longer than the signal (trimmed
    to the taps that overlap it), and nsig + taps - 1 landing exactly on a power of two and one beyond it."""
    data = _cwt64_data(3, 1200, 2)
    cases = [(5, np.array([0.001, 0.0008]), 16), (120, np.array([0.3, 0.05]), None)]
    taps = cwt64_taps(1000, [0.02], 1e-3)[0][0].size
    assert taps < 500
    cases += [(512 - taps + 1, np.array([0.02, 0.005]), 512), (512 - taps + 2, np.array([0.02, 0.005]), 1024)]
    for nsig, scales, L in cases:
        Lp = CD.cwt_conv_length64(nsig, [h.size for h, _ in cwt64_taps(nsig, scales, 1e-3)])
        if L is not None:
            assert Lp == L, (nsig, Lp, L)
        else:
            assert cwt64_taps(nsig, scales, 1e-3)[0][0].size < O.cwt_kernel(scales[0], 1e-3).size
        ss = np.array([40, 0])
        for output in ("fourier", "pow"):
            got = CD.cwt64_exec(data, ss, ss, ss + nsig, nsig, scales, 1e-3, detrend=0, output=output)
            ref = _cwt64_ref(data, ss, ss, ss + nsig, nsig, scales, 0, output)
            assert_cwt64(got, ref, output, f"cwt64 nsig {nsig} L {Lp} {output}")


@pytest.mark.parametrize("nseg,nchan,chunk", [(1, 7, 1), (7, 1, 5), (3, 3, 2)])
def test_cwt64_kernel_launches_and_chunks(nseg, nchan, chunk):
    """(segment, channel) items in launches of 3 (wg0 > 0, a ragged last launch) and segments in chunks (seg0 > 0, the
    trend and segment tables offset per chunk), stored per segment and summed over the segments (accumulate 2)."""
    nsig = 150
    data = _cwt64_data(nseg * 10 + nchan, nseg * nsig + 50, nchan)
    ss = np.arange(nseg) * nsig + 20
    lo, hi = ss - 20, ss + nsig + 10
    scales = np.array([0.01, 0.004])
    for output in ("fourier", "real"):
        ref = _cwt64_ref(data, ss, lo, hi, nsig, scales, 0, output)
        got = CD.cwt64_exec(data, ss, lo, hi, nsig, scales, 1e-3, detrend=0, output=output, per_launch=3, seg_chunk=chunk)
        assert_cwt64(got, ref, output, f"cwt64 launches of 3, chunks of {chunk}, {output}")
        tot = CD.cwt64_exec(data, ss, lo, hi, nsig, scales, 1e-3, detrend=0, output=output, per_launch=3, seg_chunk=chunk,
                           accumulate=2)
        r = ref.astype(np.complex128)
        assert_cwt64(tot, r.sum(axis=0, keepdims=True), output, f"cwt64 trial sum, {output}", nterms=nseg,
                     scale=np.abs(r).sum(axis=0, keepdims=True))


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_cwt64_kernel_selection_and_accumulation(output):
    """Post-selection (tpos, slots with gaps and unused samples): selected samples land in their slots, the others stay
    untouched; accumulate 1 adds segment b to out[b]."""
    nsig, nchan = 190, 4
    data = _cwt64_data(7, 2 * nsig + 30, nchan)
    ss = np.array([5, nsig + 20])
    scales = np.array([0.015, 0.0035])
    keep = np.r_[0:3, 10:150:7, 189]
    tpos = np.full(nsig, -1, dtype=np.int32)
    tpos[keep] = 2 * np.arange(keep.size) + 1                       # odd slots only
    nto = 2 * keep.size + 1
    ref = _cwt64_ref(data, ss, ss, ss + nsig, nsig, scales, 0, output)
    got = CD.cwt64_exec(data, ss, ss, ss + nsig, nsig, scales, 1e-3, detrend=0, output=output, tpos=tpos, ntime_out=nto)
    assert_cwt64(got[:, 1::2], ref[:, keep], output, f"cwt64 tpos {output}")
    assert not got[:, 0::2].any()
    rng = np.random.default_rng(1)
    base = rng.normal(size=got.shape).astype(got.dtype)
    if output == "fourier":
        base = base + 1j * rng.normal(size=got.shape).astype(np.float32)
    acc = CD.cwt64_exec(data, ss, ss, ss + nsig, nsig, scales, 1e-3, detrend=0, output=output, tpos=tpos, ntime_out=nto,
                       accumulate=1, out=base.copy(), seg_chunk=1)
    assert np.array_equal(acc[:, 0::2], base[:, 0::2])
    b = base[:, 1::2].astype(np.complex128)
    r = ref[:, keep].astype(np.complex128)
    assert_cwt64(acc[:, 1::2] - b, r, output, f"cwt64 accumulate 1 {output}", scale=np.abs(r) + np.abs(b + r))


def test_cwt64_kernel_wide_transposition():
    """A real output with nsig % 4 == 0 and nsig >= 1024: cwt.hip transposes it with cwt_scatter_wide_kernel."""
    nsig = 1024
    data = _cwt64_data(2, nsig + 8, 3)
    ss = np.array([4])
    scales = np.array([0.006])
    for output, acc in (("pow", 0), ("imag", 2)):
        got = CD.cwt64_exec(data, ss, ss - 4, ss + nsig + 4, nsig, scales, 1e-3, detrend=0, output=output, accumulate=acc)
        ref = _cwt64_ref(data, ss, ss - 4, ss + nsig + 4, nsig, scales, 0, output)
        assert_cwt64(got, ref, output, f"cwt64 wide transposition {output}")


def test_cwt_direct_bound():
    """cwt_direct_fits (cwt_route.h), the plan-creation rule for the direct kernels: slots increasing with the samples,
    and every tile's slot span * rowb + channel bytes below 2^32 (32-bit store offsets from the tile's reference slot)."""
    lim = 1 << 32
    # contiguous slots: the span of a full block is V - 1; a ragged last block spans less
    V, chanb = 1000, 256
    rowb = (lim - chanb) // 999
    assert CD.cwt_direct_fits(None, 5000, [V], rowb, chanb)
    assert not CD.cwt_direct_fits(None, 5000, [V], rowb + 1, chanb)
    assert CD.cwt_direct_fits(None, 1500, [V], rowb, chanb)                # (the ragged last tile spans 499)
    assert not CD.cwt_direct_fits(None, 1500, [2000], rowb, chanb)         # one tile of 1500 samples spans 1499
    assert CD.cwt_direct_fits(None, 1500, [2000], (lim - chanb) // 1499, chanb)
    # gapped slots tpos[n] = 10000 n: a 1004-sample tile spans 10 030 000 slots
    tp = (10000 * np.arange(2048)).astype(np.int32)
    assert CD.cwt_direct_fits(tp, 2048, [1004], 256, 32)                   # 2.57e9 bytes
    assert not CD.cwt_direct_fits(tp, 2048, [1004], 512, 64)               # 5.14e9 bytes
    assert not CD.cwt_direct_fits(tp, 2048, [2000, 1004], 256, 32)         # a second group with longer tiles
    span = 10000 * 1003
    assert CD.cwt_direct_fits(tp, 2048, [1004], (lim - 64) // span, 64)
    assert not CD.cwt_direct_fits(tp, 2048, [1004], (lim - 64) // span + 1, 64)
    # unmapped samples: the tile's reference is the slot reached before it (0 before any) - the second tile [1004, 2008)
    # spans 4e6 + 507 * 10000 slots from slot 0 though only its last 508 samples are mapped
    tq = np.full(2048, -1, dtype=np.int32)
    tq[1500:] = 10000 * np.arange(548) + 4000000
    assert not CD.cwt_direct_fits(tq, 2048, [1004], 512, 64)
    assert CD.cwt_direct_fits(tq, 2048, [1004], 256, 32)
    tq[1500:] -= 4000000 - 5000
    assert CD.cwt_direct_fits(tq, 2048, [1004], 512, 64)
    # slots not increasing
    assert not CD.cwt_direct_fits(np.r_[0, 2, 1].astype(np.int32), 3, [1004], 8, 8)
    assert not CD.cwt_direct_fits(np.r_[0, 1, 1].astype(np.int32), 3, [1004], 8, 8)
    assert CD.cwt_direct_fits(np.r_[0, -1, 1].astype(np.int32), 3, [1004], 8, 8)
    # production shape (c4: 128 channels, 25 scales, complex): nowhere near
    assert CD.cwt_direct_fits(None, 16384, [1004, 1900], 25 * 128 * 8, 128 * 8)


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_cwt_direct_kernels_gapped_slots(output):
    """cwt2d_kernel with slots far apart (tpos[n] = 7 n + 3, below the 32-bit bound): every sample in its slot, the slots
    between untouched - zero after a store, the old values after accumulate 1."""
    rng = np.random.default_rng(4)
    nsig, nchan = 1400, 3
    data = rng.normal(size=(2 * nsig + 30, nchan)).astype("f4") + 1.5
    ss = np.array([10, nsig + 20])
    lo, hi = ss.copy(), ss + nsig
    scales = np.array([0.012, 0.004])
    tpos = (7 * np.arange(nsig) + 3).astype(np.int32)
    nto = 7 * nsig + 5
    ref = np.stack([O.convert_output(O.cwt(O.detrend(np.array(data[a:a + nsig]), 0), 1000.0, scales).transpose(1, 0, 2), output)
                    for a in ss])
    out = CD.cwt_exec(data, ss, lo, hi, nsig, scales, 1e-3, 6.0, 0, output, tpos=tpos, ntime_out=nto)
    assert_parity(out[:, tpos], ref, what="direct cwt, gapped slots")
    gap = np.ones(nto, dtype=bool)
    gap[tpos] = False
    assert not out[:, gap].any()
    base = np.full(out.shape, 0.25, dtype=out.dtype)
    acc = CD.cwt_exec(data, ss, lo, hi, nsig, scales, 1e-3, 6.0, 0, output, tpos=tpos, ntime_out=nto,
                     accumulate=1, out=base.copy())
    assert np.array_equal(acc[:, gap], base[:, gap])
    assert_parity(acc[:, tpos] - base[:, tpos], ref, what="direct cwt, gapped slots, accumulate 1")


@pytest.mark.parametrize("n", [32, 37, 70])
def test_blocked_inverse(n):
    """Block Gauss-Jordan inverse (16 x 16 diagonal blocks): ragged sizes, identity padding, tiny-pivot flag.  The route
    gives this kernel below 64 channels, and at 70 where 64 KiB of LDS do not hold the 32-row kernel's row block."""
    rng = np.random.default_rng(n)
    B = 2
    A = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n)) + 3 * np.sqrt(n) * np.eye(n)
    kw = dict(blocked=True, lds_per_block=64 * 1024, kernel="spywil::zinv_blocked_kernel")
    inv, info = GD.inv(A, **kw)
    assert not info.any()
    np.testing.assert_allclose(inv @ A, np.tile(np.eye(n), (B, 1, 1)), atol=1e-10)
    P = np.zeros((1, n, n), complex)
    P[0] = np.eye(n)[::-1]                     # anti-diagonal permutation: every leading block is singular
    _, info = GD.inv(P, **kw)
    assert info[0] == 2


@pytest.mark.parametrize("n", [64, 65, 70, 97])
def test_blocked_inverse_on_f64_matrix_cores(n):
    """zinv_mfma_kernel (32 x 32 blocks, R = D A_k* and the trailing update as v_mfma_f64_16x16x4_f64 tiles): ragged
    sizes (identity padding, partial tiles; 65: one row in the last block), asymmetric complex matrices (a row/column
    swap of a fragment layout would show), the tiny-pivot flag.  Sizes the route sends to this kernel (64 ... 127)."""
    rng = np.random.default_rng(n)
    B = 2
    A = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n)) + 3 * np.sqrt(n) * np.eye(n)
    inv, info = GD.inv(A, blocked=True, kernel="spywil::zinv_mfma_kernel")
    assert not info.any()
    np.testing.assert_allclose(inv, np.linalg.inv(A), rtol=1e-9, atol=1e-11)
    P = np.zeros((1, n, n), complex)
    P[0] = np.eye(n)[::-1]
    _, info = GD.inv(P, blocked=True, kernel="spywil::zinv_mfma_kernel")
    assert info[0] == 2


@pytest.mark.parametrize("n", [128, 176, 192, 161])
def test_blocked_inverse_with_64_row_blocks(n):
    """zinv64_mfma_kernel (64 x 64 diagonal blocks, the matrix walked in column quarters through a 64 x 64 R panel in
    LDS, the quarter of the block itself last): ragged sizes (161: one row in the last block, 176: a whole 16-row tile
    of padding), asymmetric complex matrices, out of place, the tiny-pivot flag.  Sizes the route sends to this kernel
    (from 128 on, where 64-row blocks pad no more than 32-row blocks)."""
    rng = np.random.default_rng(n)
    B = 1 if n > 128 else 2            # (one OS thread per GPU thread: 192 x 192 costs 20 s per matrix)
    A = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n)) + 3 * np.sqrt(n) * np.eye(n)
    inv, info = GD.inv(A, blocked=True, kernel="spywil::zinv64_mfma_kernel")
    assert not info.any()
    np.testing.assert_allclose(inv, np.linalg.inv(A), rtol=1e-9, atol=1e-11)
    P = np.zeros((1, n, n), complex)
    P[0] = np.eye(n)[::-1]
    _, info = GD.inv(P, blocked=True, kernel="spywil::zinv64_mfma_kernel")
    assert info[0] == 2


@pytest.mark.parametrize("F", [9, 17, 11, 8])       # L = 16 (4*4), 32 (4*4*2), 20 (4*5), 14 (2*7)
def test_plus_operator(F):
    rng = np.random.default_rng(F)
    n, L = 3, 2 * (F - 1)
    g = rng.normal(size=(F, n, n)) + 1j * rng.normal(size=(F, n, n))
    full = np.zeros((L, n, n), complex)
    full[:F] = g
    full[F:] = np.conj(g[1:F - 1][::-1])
    ref, ref0 = O.plus_operator(full)
    gp, g0 = GD.plus(g, kernel="spywil::plus_kernel")
    np.testing.assert_allclose(gp, ref[:F], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g0, ref0, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("F,n", [(129, 3), (257, 2), (513, 5), (1025, 2), (2049, 2)])
def test_plus_operator_two_entries_per_transform(F, n):
    """plus4_kernel: two real lag sequences per complex radix-16 transform, four adjacent entries per workgroup
    (n = 3, 5: ragged last workgroup / odd pair), complex DC and Nyquist bins (their imaginary parts must be
    ignored as real(ifft(.)) ignores them) - against the oracle's fft/ifft formulation and the radix-4 kernel."""
    rng = np.random.default_rng(F + n)
    L = 2 * (F - 1)
    g = rng.normal(size=(F, n, n)) + 1j * rng.normal(size=(F, n, n))
    full = np.zeros((L, n, n), complex)
    full[:F] = g
    full[F:] = np.conj(g[1:F - 1][::-1])
    ref, ref0 = O.plus_operator(full)
    gp, g0 = GD.plus(g, kernel="spywil::plus4_kernel<%d>" % (L.bit_length() - 1))
    np.testing.assert_allclose(gp, ref[:F], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g0, ref0, rtol=1e-12, atol=1e-12)
    old, old0 = GD.plus(g, generic=True, kernel="spywil::plus_kernel")
    np.testing.assert_allclose(gp, old, rtol=1e-12, atol=1e-12)


def test_zgemm_on_f64_matrix_cores():
    """n >= 48 takes the v_mfma_f64_16x16x4_f64 tiles (asymmetric operands catch row/column swaps; n = 50 leaves
    ragged tiles)."""
    rng = np.random.default_rng(50)
    n = 50
    A = rng.normal(size=(1, n, n)) + 1j * rng.normal(size=(1, n, n))
    Bm = rng.normal(size=(1, n, n)) + 1j * rng.normal(size=(1, n, n))
    np.testing.assert_allclose(GD.gemm(A, Bm, kernel="spywil::zgemm_mfma_kernel<0>"), A @ Bm, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(GD.gemm(A, Bm, opB=1, addI=1), A @ Bm.conj().transpose(0, 2, 1) + np.eye(n), rtol=1e-12,
                               atol=1e-12)
    # addI & 2: B declared lower triangular (the Cholesky factor): the zero rows above a column tile are skipped
    n = 130
    A = rng.normal(size=(1, n, n)) + 1j * rng.normal(size=(1, n, n))
    L = np.tril(rng.normal(size=(1, n, n)) + 1j * rng.normal(size=(1, n, n)))
    np.testing.assert_allclose(GD.gemm(A, L, addI=2), A @ L, rtol=1e-12, atol=1e-12)


def test_zgemm_fused_skew_and_error_check():
    """The two fused forms of the matrix-core gemm used inside the Wilson iteration: psi (g+ + S) with
    S = triu(g0) - triu(g0)^H joined to the B operand, and max_rel_err(CSD, psi psi^H) without storing the product
    (wilson_sf.py:97-101,190-194); n = 70 leaves partial 64 x 64 tiles."""
    rng = np.random.default_rng(12)
    n, B = 70, 2
    psi = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n))
    gp = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n))
    g0 = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    S, g0S = GD.skew(g0)
    Sref = np.triu(g0) - np.triu(g0).conj().T
    np.testing.assert_allclose(S, Sref, rtol=0, atol=0)
    np.testing.assert_allclose(g0S, g0 + Sref, rtol=1e-15)
    np.testing.assert_allclose(GD.gemm(psi, gp, badd=S, kernel="spywil::zgemm_mfma_kernel<1>"), psi @ (gp + Sref), rtol=1e-12, atol=1e-12)
    # X X^H + I through the Hermitian instance (lower tiles computed, mirrored above the diagonal)
    np.testing.assert_allclose(GD.gemm(psi, psi, opB=1, addI=1, kernel="spywil::zgemm_mfma_kernel<3>"),
                               psi @ psi.conj().transpose(0, 2, 1) + np.eye(n), rtol=1e-12, atol=1e-12)
    herm = rng.normal(size=(B, n, n)) * 1e-3
    ref = psi @ psi.conj().transpose(0, 2, 1) * (1 + herm + herm.transpose(0, 2, 1))        # Hermitian reference
    err = GD.gemm(psi, psi, opB=1, ref=ref, kernel="spywil::zgemm_mfma_kernel<2>")
    np.testing.assert_allclose(err, O.max_rel_err(ref, psi @ psi.conj().transpose(0, 2, 1)), rtol=1e-10)


@pytest.mark.parametrize("n", [63, 65])
def test_hermitian_zgemm_ragged_tiles(n):
    """X X^H + I through the Hermitian instance (zgemm_mfma_kernel<3>) with one ragged tile (63) and with a ragged last
    tile row whose mirror fills the column above it (65); nine matrices, so the batch is not a multiple of 8."""
    rng = np.random.default_rng(n)
    X = rng.normal(size=(9, n, n)) + 1j * rng.normal(size=(9, n, n))
    np.testing.assert_allclose(GD.gemm(X, X, opB=1, addI=1, kernel="spywil::zgemm_mfma_kernel<3>"),
                               X @ X.conj().transpose(0, 2, 1) + np.eye(n), rtol=1e-12, atol=1e-12)


def test_wilson_building_blocks():
    rng = np.random.default_rng(3)
    n, B = 37, 3
    A = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n))
    Bm = rng.normal(size=(B, n, n)) + 1j * rng.normal(size=(B, n, n))
    np.testing.assert_allclose(GD.gemm(A, Bm), A @ Bm, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(GD.gemm(A, Bm, opB=1, addI=1), A @ Bm.conj().transpose(0, 2, 1) + np.eye(n), rtol=1e-12,
                               atol=1e-12)
    np.testing.assert_allclose(GD.gemm(A, Bm[0], kernel="spywil::zgemm_kernel"), A @ Bm[0], rtol=1e-12, atol=1e-12)        # broadcast B
    inv, info = GD.inv(A, kernel="spywil::zinv_kernel")
    assert not info.any()
    np.testing.assert_allclose(inv @ A, np.tile(np.eye(n), (B, 1, 1)), atol=1e-9)
    P = A @ A.conj().transpose(0, 2, 1) + n * np.eye(n)
    Lc, info = GD.chol(P, kernel="spywil::zchol_kernel")
    assert not info.any()
    np.testing.assert_allclose(Lc, np.linalg.cholesky(P), rtol=1e-10, atol=1e-10)
    assert abs(GD.cond(P[:1, :9, :9]) / np.linalg.cond(P[0, :9, :9]) - 1) < 5e-2


@pytest.mark.parametrize("n", [64, 70])
def test_panel_cholesky(n):
    """zchol_panel_kernel (n >= 64: left-looking panels of 32 columns; 70: a ragged last panel of 6): the factor, the
    zeroed strict upper triangle, and the flag for a matrix that is not positive definite."""
    rng = np.random.default_rng(n)
    X = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
    P = X @ X.conj().transpose(0, 2, 1) + 0.5 * n * np.eye(n)
    P[2, 40, 40] = -1.0                                        # third matrix: indefinite
    Lc, info = GD.chol(P, kernel="spywil::zchol_panel_kernel")
    assert list(info) == [0, 0, 1]
    np.testing.assert_allclose(Lc[:2], np.linalg.cholesky(P[:2]), rtol=1e-10, atol=1e-10)
    assert np.all(np.triu(Lc[:2], 1) == 0)


@pytest.mark.skipif(not __import__("os").environ.get("SPY_EMU_SLOW"),
                    reason="~5 min of thread emulation; set SPY_EMU_SLOW=1 (the GPU suite covers the same chain)")
def test_wilson_granger_small_vs_oracle():
    """Whole Wilson/Granger chain on emulated kernels for a small problem (the golden-vector comparison of
    the real C++ driver runs on the GPU: tests/test_gpu_golden.py)."""
    adj = np.zeros((3, 3))
    adj[0, 1] = 0.3
    trials = O.ar2_network(adj, 32, 40, seed=3)
    acc = np.zeros((17, 3, 3), np.complex64)
    for x in trials:
        cs, _ = O.csd(O.detrend(x, 0), 200.0, 32, "dpss", {"NW": 2, "Kmax": 3}, demean_taper=True)
        acc += cs
    acc /= len(trials)
    G, H, Sigma, info = GD.granger(acc)
    Gr, meta = O.granger_cF(acc[None])
    assert bool(info[0]) == bool(meta["converged--bool"]) and info[2] == float(meta["reg. factor--float"])
    np.testing.assert_allclose(info[3], float(meta["initial cond. num--float"]), rtol=0.2)
    assert info[1] < 5e-6
    rec = H @ Sigma @ H.conj().transpose(0, 2, 1)
    assert O.max_rel_err(acc.astype(np.complex128), rec) < 1e-5
    np.testing.assert_allclose(G[2:-1], Gr[0, 2:-1], rtol=5e-3, atol=5e-4)
    np.testing.assert_allclose(G, Gr[0], atol=1e-2)


def test_reference_order_mean_is_numpy_bit_for_bit():
    """seq_mean_kernel = np.mean(float32 (time x channel), axis=0) bit for bit: NumPy reduces the slow axis with one
    float32 accumulator per channel in time order (what scipy.signal.detrend(type='constant') subtracts,
    specest/compRoutines.py:169-170).  Offsets make the rounding sequence matter; zero-extended segments, channel
    selections and channel counts around the 64-lane edge are covered."""
    rng = np.random.default_rng(7)
    x = (rng.normal(size=(5000, 70)) * rng.uniform(0.1, 30, size=70) + rng.uniform(-500, 500, size=70)).astype(np.float32)
    got = E.seq_mean(x, [0, 17, 1000], [0, 17, 1000], [4096, 17 + 3001, 1000 + 33], 4096)
    assert np.array_equal(got[0], np.mean(x[:4096], axis=0))
    assert got[0].dtype == np.float32
    # rows outside [lo, hi) count as zeros: sum over the valid rows, divided by nsig
    assert np.array_equal(got[1], np.add.reduce(x[17:17 + 3001], axis=0) / np.float32(4096))
    assert np.array_equal(got[2], np.add.reduce(x[1000:1033], axis=0) / np.float32(4096))
    ci = [69, 0, 5, 5, 64, 63]
    got = E.seq_mean(x, [3], [3], [3 + 2000], 2000, chan_idx=ci)
    assert np.array_equal(got[0], np.mean(np.ascontiguousarray(x[3:2003][:, ci]), axis=0))    # C order, as a trial is
    # the float64 block sums differ from this by up to ~1e-6 of the offset - that is the whole point
    exact = x[:4096].astype(np.float64).mean(axis=0)
    assert np.abs(np.mean(x[:4096], axis=0) - exact).max() > 1e-5
    # ONE channel: the trial is an (nSamples, 1) array, contiguous along the reduced axis, which NumPy sums pairwise
    # (pairwise_sum_FLOAT) - a different rounding sequence from the row-by-row one above
    for n in (5, 8, 100, 128, 129, 1000, 4096, 4100, 4999):
        for src in (np.ascontiguousarray(x[:n, 3:4]), x):                      # a one-channel recording / one selected column
            ci = None if src.shape[1] == 1 else [3]
            got = E.seq_mean(src, [0], [0], [n], n, chan_idx=ci)
            assert np.array_equal(got[0], np.mean(np.ascontiguousarray(x[:n, 3:4]), axis=0)), n
    seq = np.float32(0)
    for v in x[:4096, 3]:
        seq = np.float32(seq + v)
    assert seq / np.float32(4096) != np.mean(np.ascontiguousarray(x[:4096, 3:4]), axis=0)[0]    # (the orders do differ)


# (2000 forced: the route gives it its compile-time schedule; this case has always run the mixed-radix engine)
@pytest.mark.parametrize("nsig,nfft,kw", [(4096, 4096, {}), (1000, 1024, {}), (2000, 2000, {"mixed": True}),
                                          (600, 600, {"force_generic": True}), (5003, 5003, {"force_long": True}),
                                          (16384, 16384, {})])
def test_offset_channels_match_the_reference_next_to_dc(nsig, nfft, kw):
    """Every kernel family with `reference_mean`: a channel riding on an offset 1000x its fluctuations reproduces the
    oracle (float32 sequential mean, then float64 taper and FFT) within the unwidened criterion; with the float64
    block sums the bins next to DC miss it (which is why the golden tests used to carry a wider floor)."""
    rng = np.random.default_rng(nsig)
    C = 6
    x = rng.normal(size=(nsig, C)).astype(np.float32)
    x[:, 1] += 1000.0
    x[:, 4] -= 313.7
    topt = {"NW": 3, "Kmax": 4}
    tap = O.taper_table("dpss", nsig, nfft, topt)
    sc = O.spec_scale(nsig, nfft)
    ref, _ = O.mtmfft(O.detrend(x, 0), 1000.0, nfft, "dpss", topt)
    got = E.fft_exec(x, [0], [0], [nsig], nsig, nfft, tap, sc, detrend=0, output="fourier", keeptapers=True,
                     reference_mean=True, **kw)[0]
    kernel = {4096: "mtmfft_quad_kernel<12, 2, 2, false>", 1024: "mtmfft_quad_kernel<10, 4, 2, false>", 2000: "mtmfft_mixed_kernel<",
              600: "mtmfft_generic_kernel<", 5003: "mtmfft_long<128 x 128,", 16384: "mtmfft_quad_kernel<13, 1, 2, false, HALF of N = 16384>"}[nfft]
    assert E.LAST_KERNEL.startswith(kernel), E.LAST_KERNEL
    for c in range(C):                       # per channel: the criterion relative to THAT channel's largest bin
        assert_parity(got[:, :, c], ref[:, :, c], what=f"channel {c} with reference-order mean")
    plain = E.fft_exec(x, [0], [0], [nsig], nsig, nfft, tap, sc, detrend=0, output="fourier", keeptapers=True, **kw)[0]
    if nsig >= 1000:                         # (short sums happen to round well)
        assert excess(plain[:, :, 1], ref[:, :, 1]) > 1.0


# ---------------------------------------------------------------------------------------------------------------
# K1d: compile-time radix schedules (mtmfft_dec_kernel.h)
@pytest.mark.parametrize("dec,nfft,nchan,K,output,keeptapers,detrend,demean", [
    (100, 100, 68, 2, "fourier", True, 0, False),      # 10 x 10, sixteen quads per workgroup (+ one padded group)
    (400, 400, 35, 2, "pow", False, 1, False),         # 10 x 10 x 2 x 2, eight quads per workgroup
    (3200, 3200, 4, 1, "fourier", True, 0, False),     # 20 x 20 x 4 x 2
    (1000, 1000, 8, 2, "fourier", True, 0, False),     # 10 x 10 x 10, two quads per workgroup, fast stores
    (1000, 1000, 5, 3, "pow", False, 1, True),         # ragged channels, taper mean, linear detrend, demean_taper
    (2000, 2000, 4, 2, "pow", True, 0, False),         # 10 x 10 x 10 x 2: BASELINE config 1's length
    (2000, 2000, 3, 2, "fourier", False, -1, False),
    (2001, 2000, 8, 2, "abs", True, 0, False),         # 20 x 10 x 10
    (5000, 5000, 4, 1, "fourier", True, 0, False),     # 10 x 10 x 10 x 5
    (512, 512, 16, 2, "pow", True, 0, False),          # V = 8: 8 x 8 x 8
    (4096, 4096, 4, 2, "fourier", True, 0, False),     # 8 x 8 x 8 x 8
])
def test_dec_kernel_vs_oracle(dec, nfft, nchan, K, output, keeptapers, detrend, demean):
    _fft_case(nfft, nfft, nchan, K, output, keeptapers, detrend, demean_taper=demean, nseg=2 if nfft <= 1000 else 1, dec=dec)


@pytest.mark.parametrize("nfft,nchan,K,output,keeptapers,detrend,demean", [
    (600, 16, 2, "fourier", True, 0, False),           # 3 x 200, four quads per workgroup, fast stores
    (1500, 5, 3, "pow", False, 1, True),               # 3 x 500: ragged channels, taper mean, linear detrend, demean_taper
    (3000, 4, 2, "fourier", True, 0, False),           # 3 x 1000
    (3000, 3, 2, "abs", False, -1, False),
    (6000, 4, 1, "pow", True, 0, False),               # 3 x 2000
    (300, 33, 2, "fourier", True, 0, False),           # 3 x 100, eight quads per workgroup
    (2400, 4, 2, "abs", True, 0, False),               # 3 x 800, 20 values per thread
    (768, 9, 2, "fourier", True, 0, False),            # 3 x 256, 16 values per thread
    (3072, 4, 2, "pow", False, 0, False),              # 3 x 1024
])
def test_dec_kernel_radix3_decimation(nfft, nchan, K, output, keeptapers, detrend, demean):
    # N = 3 M: three scheduled sub-transforms side by side and one radix-3 combine through LDS (CfgD::P)
    _fft_case(nfft, nfft, nchan, K, output, keeptapers, detrend, demean_taper=demean, nseg=2 if nfft <= 1500 else 1, dec=nfft)


@pytest.mark.parametrize("dec,nfft,nchan,K,output,keeptapers,detrend,demean", [
    (1001, 1000, 8, 2, "fourier", True, 0, False),     # the 1000-point schedule with split exchanges
    (1001, 1000, 5, 3, "pow", False, 1, True),
    (10000, 10000, 4, 1, "fourier", True, 0, False),   # 20 x 20 x 5 x 5, 500 threads
    (10000, 10000, 3, 2, "pow", False, 0, False),
])
def test_dec_kernel_split_exchanges(dec, nfft, nchan, K, output, keeptapers, detrend, demean):
    _fft_case(nfft, nfft, nchan, K, output, keeptapers, detrend, demean_taper=demean, nseg=2 if nfft <= 1000 else 1, dec=dec)


def test_dec_kernel_radix3_padding_and_selection():
    _fft_case(2700, 3000, 6, 2, "pow", True, 0, dec=3000, nseg=1, freq_idx=np.array([0, 1, 1499, 1500, 37, 1000, 1001]),
              chan_idx=np.array([5, 0, 2, 2]))
    _fft_case(1400, 1500, 4, 2, "fourier", True, 1, dec=1500, nseg=2)


@pytest.mark.parametrize("P,M,nsig,nchan,K,output,keeptapers,detrend,demean,refmean", [
    (6, 2000, 12000, 5, 2, "fourier", True, 0, False, True),       # ragged quads, reference-order mean
    (6, 2000, 11000, 4, 2, "pow", False, 1, True, False),          # zero padding, line fit and demean_taper from the statistics
    (3, 4096, 12288, 3, 1, "abs", True, -1, False, False),         # 16 values per thread in the sub-transform
    (4, 5000, 20000, 2, 1, "fourier", False, 0, False, True),      # radix 4: the factors +-1, +-i
])
def test_long_trials_through_scratch_memory(P, M, nsig, nchan, K, output, keeptapers, detrend, demean, refmean):
    """K1L2 (mtmfft_declong.h): N = P M beyond one workgroup's LDS - statistics, scheduled sub-transforms of the samples
    P m + r, radix-P step + separation + conversion, against the oracle."""
    nfft = P * M
    rng = np.random.default_rng(P * M + nchan)
    data = (rng.normal(size=(nsig + 9, nchan)) + (5.0 if detrend == 0 else 0.0)).astype("f4")
    ss = np.array([4])
    taper, topt = ("dpss", {"NW": (K + 1) / 2, "Kmax": K}) if K > 1 else ("hann", {})
    tapers = O.taper_table(taper, nsig, nfft, topt)
    fi = np.array([0, 1, M - 1, M, M + 1, nfft // 2 - 1, nfft // 2, 37]) if output == "abs" else None
    out = E.fft_exec_declong(data, ss, ss, ss + nsig, nsig, P, M, tapers, O.spec_scale(nsig, nfft), detrend, demean, fi, output,
                             keeptapers, reference_mean=refmean)
    freqs = np.fft.rfftfreq(nfft, 1e-3)
    ref, _ = O.mtmfft_cF(np.array(data[4:4 + nsig]), foi=freqs if fi is None else freqs[fi], keeptapers=keeptapers,
                         polyremoval=None if detrend < 0 else detrend, output=output,
                         method_kwargs=dict(samplerate=1000.0, taper=taper, taper_opt=topt, nSamples=nfft, demean_taper=demean))
    assert_parity(out[0], ref[0], what=f"{P} x {M}")


@pytest.mark.parametrize("nsig,nfft,nchan,K,output,keeptapers,detrend,demean", [
    (2000, 2000, 8, 2, "fourier", True, 0, False),     # pairs through 10 x 10 x 10, two pairs per workgroup, fast stores
    (2000, 2000, 5, 3, "pow", False, 1, True),         # ragged channels, taper mean, line fit over even + odd samples, demean_taper
    (1999, 2000, 3, 2, "abs", True, 0, False),         # odd sample count: the last pair is half padding
    (1501, 2000, 4, 2, "fourier", False, -1, False),   # zero padding, complex taper mean
    (2000, 2002, 6, 2, "fourier", True, 0, False),     # ... with split exchanges (id 2002 = the 1000-point schedule, SPLIT)
    (1200, 1200, 9, 2, "fourier", True, 0, True),      # 3 x 200: radix-3 decimation in front, four pairs per workgroup
    (1100, 1200, 4, 3, "pow", False, 1, False),
    (1024, 1024, 6, 2, "pow", True, 0, False),         # 16 x 16 x 2
    (5000, 5000, 4, 1, "pow", True, 0, False),         # 10 x 10 x 5 x 5 (the product's choice for nfft = 5000)
    (12000, 12000, 2, 1, "fourier", True, 0, False),   # 3 x (10 x 10 x 10 x 2): trials beyond a quad's LDS
])
def test_dec_kernel_half_form(nsig, nfft, nchan, K, output, keeptapers, detrend, demean):
    """CfgD::HALF: z[m] = x[2 m] + i x[2 m + 1] through the length-nfft/2 schedule, bins f and nfft/2 - f from Z[f], Z[nfft/2 - f]."""
    real_nfft = 2000 if nfft == 2002 else nfft
    _fft_case(nsig, real_nfft, nchan, K, output, keeptapers, detrend, demean_taper=demean, nseg=2 if nfft <= 2002 else 1, dec=-nfft)


def test_dec_kernel_half_form_selection():
    _fft_case(1700, 2000, 6, 2, "pow", True, 0, dec=-2000, nseg=1, freq_idx=np.array([0, 1, 999, 1000, 37, 500, 501, 499]),
              chan_idx=np.array([5, 0, 2, 2, 1]))
    _fft_case(1200, 1200, 3, 2, "fourier", False, 0, dec=-1200, nseg=1, freq_idx=np.array([600, 0, 300, 299, 301, 200, 400]))


def test_dec_kernel_padding_and_selection():
    _fft_case(1700, 2000, 6, 2, "pow", True, 0, dec=2000, nseg=1, freq_idx=np.array([0, 1, 999, 1000, 37]),
              chan_idx=np.array([5, 0, 2, 2]))
    _fft_case(900, 1000, 4, 2, "fourier", True, 1, dec=1000, nseg=2)


def test_csd_3m_more_than_512_channels():
    """More than 512 channels (csd.hip): Hermitian 3M products of the 256-channel blocks + the rectangle kernel
    (csd3m_kernel<512, 8, false, true>: two channel ranges side by side in one LDS image) for every pair of blocks; an odd
    count sends its last row through the rank-1 update.  520 channels = blocks of 256, 256, 8."""
    C, F, R = 521, 1, 6
    rng = np.random.default_rng(3)
    spec = (rng.normal(size=(R, F, C)) + 1j * rng.normal(size=(R, F, C))).astype(np.complex64)
    acc = np.zeros((F, C, C), np.complex64)
    few = dict(workgroups=8)          # the rank-1 update strides over 8 workgroups (of 256 OS threads each here), not 1061
    assert D.csd_accumulate(spec[:2], acc, **few) == 10 and D.csd_accumulate(spec[2:], acc, **few) == 10
    ref = np.einsum("rfi,rfj->fij", spec.astype(np.complex128), spec.conj().astype(np.complex128))
    ii, jj = np.tril_indices(C)
    assert_parity(acc[:, ii, jj], ref[:, ii, jj].astype(np.complex64), what="wide csd, lower triangle")
    iu, ju = np.triu_indices(C, 1)
    off = iu // 16 != ju // 16                           # (a diagonal 16 x 16 tile is stored whole, as for <= 512)
    assert not acc[:, iu[off], ju[off]].any()            # nothing else lands above the diagonal
    # phase-exact accumulation: the same walk with the 4-multiplication instances (csd3m_kernel<..., M4 = true>)
    acc4 = np.zeros((F, C, C), np.complex64)
    assert D.csd_accumulate(spec, acc4, force_4m=True, **few) == 11
    assert_parity(acc4[:, ii, jj], ref[:, ii, jj].astype(np.complex64), what="wide csd, 4 multiplications")
    # its imaginary part is a sum of products, not a difference of the three 3M products: error ~ eps * |Im| terms only
    coherent = np.repeat(spec[:, :, :1], C, axis=2) * (1 + 1e-3 * rng.normal(size=(1, 1, C))).astype(np.float32)
    acc4[:] = 0
    D.csd_accumulate(coherent.astype(np.complex64), acc4, force_4m=True, **few)
    scale = np.abs(acc4[0, 0, 0])
    assert np.abs(acc4[:, ii, jj].imag).max() <= 1e-6 * scale       # real multiples of one signal: Im = 0 up to rounding


# K1r second generation: reference-precision transforms (mtmfft_dec64_kernel.h, mtmfft_f64_kernel.h incl. Bluestein)
def _f64_case(nsig, nfft, nchan, K, output, keeptapers, detrend, demean_taper=False, freq_idx=None, chan_idx=None, nseg=1,
              seed=3, dec=None, bluestein=None, pure_frac=0.99, emu_id=None, kernel=None):
    """Data with 60 dB of dynamic range (a 40 Hz line 1000 x the noise, an offset): the criterion everywhere, and for
    complex output PURE rtol 1e-5 bin by bin on >= 99 % of the bins - which only a float64 transform delivers.
    The family is the one spyfft::fft_route64 gives nfft, and `kernel` the prefix of its name - by default the compile-time
    schedule of nfft; dec=True / dec="half" / bluestein=False force a family (emu_driver.fft_exec_f64)."""
    if kernel is None:
        kernel = f"mtmfft_dec64_kernel<HALF of N = {nfft}," if dec == "half" else f"mtmfft_dec64_kernel<N = {nfft},"
    rng = np.random.default_rng(seed)
    t = np.arange(nsig * nseg + 9) / 1000.0
    data = (rng.normal(size=(nsig * nseg + 9, nchan)) + 1000.0 * np.sin(2 * np.pi * 40.0 * t)[:, None] + 50.0).astype("f4")
    ss = np.array([4 + i * nsig for i in range(nseg)])
    taper, topt = ("dpss", {"NW": (K + 1) / 2, "Kmax": K}) if K > 1 else ("hann", {})
    tapers = O.taper_table(taper, nsig, nfft, topt)
    out = E.fft_exec_f64(data, ss, ss, ss + nsig, nsig, nfft, tapers, O.spec_scale(nsig, nfft), detrend, demean_taper,
                         freq_idx, output, keeptapers, chan_idx=chan_idx, reference_mean=True, dec=dec, bluestein=bluestein,
                         emu_id=emu_id)
    assert E.LAST_KERNEL.startswith(kernel), (E.LAST_KERNEL, kernel)
    freqs = np.fft.rfftfreq(nfft, 1e-3)
    foi = freqs if freq_idx is None else freqs[freq_idx]
    for b in range(nseg):
        x = data[ss[b]:ss[b] + nsig]
        if chan_idx is not None:
            x = x[:, chan_idx]
        ref, _ = O.mtmfft_cF(np.array(x, order="C"), foi=foi, keeptapers=keeptapers, polyremoval=None if detrend < 0 else detrend,
                             output=output, method_kwargs=dict(samplerate=1000.0, taper=taper, taper_opt=topt,
                                                               nSamples=nfft, demean_taper=demean_taper))
        assert_parity(out[b], ref[0], what=f"segment {b}")
        if output == "fourier" and detrend != 1:
            err = np.abs(out[b].astype(np.complex128) - ref[0])
            frac = float((err <= 1e-5 * np.abs(ref[0])).mean())
            assert frac >= pure_frac, (nfft, frac)


@pytest.mark.parametrize("nfft,nchan,K", [(256, 33, 2), (1024, 9, 2), (4096, 3, 2),
                                          (200, 17, 2), (1000, 5, 2), (2000, 3, 2), (2500, 2, 1)])
def test_dec64_kernel_vs_oracle(nfft, nchan, K):
    _f64_case(nfft, nfft, nchan, K, "fourier", True, 0)


@pytest.mark.parametrize("nfft", [8192, 16384, 4000, 5000, 10000])
def test_dec64_kernel_long_schedules(nfft):
    # 8192: four passes; 16384: 1024 threads, split exchange, samples re-read per taper; 10000: split exchange, V = 20
    # (16384 forced: the route gives it the HALF form, single channels through the schedule of 8192)
    _f64_case(nfft, nfft, 2, 1, "fourier", True, 0, dec=True if nfft == 16384 else None)


@pytest.mark.parametrize("nfft,nchan,K", [(100, 35, 2), (300, 17, 2), (400, 9, 2), (2400, 3, 1), (3200, 2, 1), (600, 9, 2), (768, 5, 2), (1500, 5, 2), (3000, 3, 2), (3072, 2, 1), (6000, 2, 1),
                                          (7500, 2, 1)])
def test_dec64_kernel_radix3_decimation(nfft, nchan, K):
    # N = 3 M: three scheduled sub-transforms side by side and one radix-3 combine through LDS (CfgD64::P)
    _f64_case(nfft, nfft, nchan, K, "fourier", True, 0)


def test_dec64_kernel_radix3_options():
    _f64_case(2800, 3000, 3, 2, "pow", False, 1)                                  # padding, linear trend, taper mean
    _f64_case(1400, 1500, 5, 2, "abs", True, 0, freq_idx=np.array([0, 1, 749, 750, 37, 500, 501]), chan_idx=[4, 0, 3])
    _f64_case(600, 600, 7, 3, "fourier", False, -1, demean_taper=True, nseg=2)    # complex taper mean, demean_taper
    _f64_case(3000, 3000, 1, 2, "pow", True, 0)                                   # a single channel: half a pair


def test_dec64_kernel_options():
    _f64_case(900, 1000, 4, 2, "pow", False, 1)                                   # padding, linear trend, taper mean
    _f64_case(1700, 2000, 6, 2, "abs", True, 0, freq_idx=np.array([0, 1, 999, 1000, 37]), chan_idx=[5, 0, 3])
    _f64_case(256, 256, 7, 3, "fourier", False, -1, demean_taper=True, nseg=2)    # complex taper mean, demean_taper
    _f64_case(900, 1024, 2, 1, "imag", True, 0, nseg=2)
    _f64_case(4096, 4096, 1, 2, "pow", True, 0)                                   # a single channel: half a pair


@pytest.mark.parametrize("nsig,nfft,nchan,K,output,keeptapers,detrend,demean,emu_id", [
    (2000, 2000, 5, 2, "fourier", True, 0, False, None),     # single channels through 10 x 10 x 10, two per workgroup
    (2000, 2000, 3, 3, "pow", False, 1, True, None),         # taper mean, line fit over even + odd samples, demean_taper
    (1999, 2000, 2, 2, "abs", True, 0, False, None),         # odd sample count: the last pair is half padding
    (1501, 2000, 3, 2, "fourier", False, -1, False, None),   # zero padding, complex taper mean
    (2000, 2000, 4, 2, "fourier", True, 0, False, 2002),     # split exchanges
    (1200, 1200, 5, 2, "fourier", True, 0, True, None),      # 3 x 200: radix-3 decimation in front
    (1100, 1200, 3, 2, "pow", False, 1, False, None),
    (1024, 1024, 3, 2, "pow", True, 0, False, None),         # powers from the table (no hoisted base twiddles)
    (12000, 12000, 1, 1, "fourier", True, 0, False, None),   # the product's schedule for nfft = 12000: un-forced
])
def test_dec64_kernel_half_form(nsig, nfft, nchan, K, output, keeptapers, detrend, demean, emu_id):
    """CfgD64::HALF: one channel = one complex128 transform of (even, odd) samples through the schedule of nfft / 2."""
    _f64_case(nsig, nfft, nchan, K, output, keeptapers, detrend, demean_taper=demean, nseg=2 if nfft <= 2000 else 1,
              dec=None if nfft == 12000 else "half", emu_id=emu_id, kernel=f"mtmfft_dec64_kernel<HALF of N = {nfft},")


def test_dec64_kernel_half_form_selection():
    _f64_case(1700, 2000, 5, 2, "pow", True, 0, dec="half", freq_idx=np.array([0, 1, 999, 1000, 37, 500, 501, 499]),
              chan_idx=np.array([4, 0, 2, 2]))
    _f64_case(1200, 1200, 3, 2, "fourier", False, 0, dec="half", freq_idx=np.array([600, 0, 300, 299, 301, 200, 400]))


@pytest.mark.parametrize("nfft,nchan,K,bluestein", [(360, 3, 2, False), (1009, 2, 1, True), (134, 3, 2, True),
                                                     (3001, 1, 1, True), (268, 2, 1, False)])
def test_f64_any_kernel_and_bluestein_vs_oracle(nfft, nchan, K, bluestein):
    # 1009 and 3001 are primes, 134 = 2 x 67, 268 = 4 x 67 through the O(R^2) pass AND through the chirp-z form
    # (the route takes the chirp-z form beyond a prime factor of 61: 268 without it is forced)
    name = f"mtmfft_f64_any_kernel<2, false> N={nfft}"
    _f64_case(nfft, nfft, nchan, K, "fourier", True, 0, bluestein=False if nfft == 268 else bluestein or None,
              kernel=name + " (Bluestein, M = " if bluestein else name)
    assert ("Bluestein" in E.LAST_KERNEL) == bluestein
    if nfft == 268:
        _f64_case(nfft, nfft, nchan, K, "fourier", True, 0, bluestein=True, kernel=name + " (Bluestein, M = 1024)")
