"""Parity of the HIP kernels (through the C ABI) against the oracle on seeded inputs."""
import numpy as np
import pytest

from oracle import spy_oracle as O
from parity import assert_parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


def _run_fft(be, data, nsig, nfft, taper, topt, output, keeptapers, detrend, demean_taper=False, freq_idx=None,
             chan_idx=None, starts=None):
    nchan = data.shape[1] if chan_idx is None else len(chan_idx)
    tapers = O.taper_table(taper, nsig, nfft, topt)
    scale = O.spec_scale(nsig, nfft)
    plan = be.FFTPlan(nsig, nfft, nchan, tapers, scale, detrend, demean_taper, freq_idx, output, keeptapers)
    d = torch.from_numpy(data).cuda()
    ss = torch.tensor(starts, dtype=torch.int64, device="cuda")
    ci = None if chan_idx is None else torch.tensor(chan_idx, dtype=torch.int32, device="cuda")
    out = plan.execute(d, ss, chan_idx=ci)
    torch.cuda.synchronize()
    return out.cpu().numpy(), plan


def _oracle_fft(data, starts, nsig, nfft, taper, topt, output, keeptapers, detrend, demean_taper, freq_idx, chan_idx):
    freqs = np.fft.rfftfreq(nfft, 1 / 1000.0)
    foi = freqs if freq_idx is None else freqs[freq_idx]
    res = []
    for s in starts:
        x = data[s:s + nsig]
        if chan_idx is not None:
            x = x[:, chan_idx]
        r, _ = O.mtmfft_cF(np.array(x), foi=foi, keeptapers=keeptapers, polyremoval=detrend, output=output,
                           method_kwargs=dict(samplerate=1000.0, taper=taper, taper_opt=topt, nSamples=nfft,
                                              demean_taper=demean_taper))
        res.append(r)
    return np.concatenate(res, axis=0)


CASES = [
    # nsig, nfft, C, taper, topt, output, keeptapers, detrend, demean_taper
    (256, 256, 6, "hann", {}, "pow", True, 0, False),
    (500, 512, 9, "dpss", {"NW": 2.5, "Kmax": 4}, "pow", False, 0, False),
    (1000, 1024, 5, "dpss", {"NW": 2, "Kmax": 3}, "fourier", True, 1, False),
    (2048, 2048, 16, "dpss", {"NW": 4, "Kmax": 7}, "pow", False, 0, True),
    (4096, 4096, 32, "dpss", {"NW": 4.096, "Kmax": 7}, "pow", False, 0, False),
    (4096, 4096, 7, "dpss", {"NW": 4.096, "Kmax": 7}, "fourier", True, 0, True),
    (5000, 8192, 4, "hann", {}, "abs", True, None, False),
    (16384, 16384, 3, "dpss", {"NW": 3, "Kmax": 5}, "pow", False, 0, False),
    (2000, 2000, 16, "dpss", {"NW": 4, "Kmax": 7}, "pow", False, 0, False),          # BASELINE config 1 shape
    (500, 500, 8, "hann", {}, "pow", True, 0, False),
    # long transforms (Bluestein + four-step FFTs through HBM): not powers of two above 4096, anything above 16384
    (5003, 5003, 6, "dpss", {"NW": 3, "Kmax": 3}, "pow", False, 1, True),             # prime
    (11000, 11000, 4, "hann", {}, "fourier", True, 0, False),
    (5000, 5000, 6, "dpss", {"NW": 3, "Kmax": 3}, "pow", False, 1, True),             # 8*5^4: mixed-radix LDS kernel
    (32768, 32768, 3, "dpss", {"NW": 2, "Kmax": 2}, "pow", False, 0, False),           # power of two: declong<8 x 4096>
    (30000, 30000, 5, "dpss", {"NW": 2, "Kmax": 2}, "abs", True, 0, False),
    (20000, 32768, 2, "hann", {}, "pow", True, None, False),
    # 10240 < N <= 20480: channel PAIRS through the compile-time schedule of N / 2 (CfgD::HALF, mtmfft_dec_{m,n}.hip);
    # the reference-precision twins of these lengths are HALF schedules too (single channels, CfgD64::HALF)
    (12000, 12000, 6, "dpss", {"NW": 3, "Kmax": 3}, "fourier", True, 1, True),        # 3 x 2000 pairs, line fit, demean_taper
    (12288, 12288, 5, "dpss", {"NW": 2, "Kmax": 2}, "pow", False, 0, False),          # 3 x 2048, odd channel count
    (15000, 15000, 7, "hann", {}, "abs", True, 0, False),                              # 3 x 2500
    (14000, 16000, 4, "dpss", {"NW": 2, "Kmax": 2}, "fourier", False, 0, False),      # 8000, zero padding, complex taper mean
    (20000, 20000, 3, "hann", {}, "pow", True, None, False),                           # 10000: split exchanges
    (11999, 12000, 3, "dpss", {"NW": 2, "Kmax": 2}, "pow", True, 1, True),             # odd sample count: the last pair is half padding
    (16001, 16384, 2, "hann", {}, "fourier", True, 0, True),
    # N = P M through HBM (mtmfft_declong.h): scheduled sub-transforms of length M, one radix-P pass, P = 2 ... 8
    (24000, 24000, 2, "hann", {}, "fourier", True, 0, False),                          # 6 x 4000
    (30000, 30000, 5, "hann", {}, "pow", False, 1, True),                              # 6 x 5000, line fit, demean_taper
    (50000, 50000, 2, "hann", {}, "pow", True, 0, False),                              # 5 x 10000
    (64000, 64000, 1, "hann", {}, "fourier", True, 0, False),                          # 8 x 8000
    (9000, 20000, 9, "dpss", {"NW": 2, "Kmax": 2}, "pow", False, 1, False),            # ragged quads, mostly padding
    (1800, 2000, 4, "dpss", {"NW": 3.6, "Kmax": 6}, "fourier", True, 1, True),
    (360, 360, 3, None, {}, "angle", True, None, False),
    (1009, 1009, 2, "hann", {}, "pow", True, 0, False),                                # prime: Bluestein
    (300, 2 * 331, 3, "hann", {}, "fourier", True, 0, False),                          # Bluestein, padded
    # 3 x a scheduled length: radix-3 decimation in front of the compile-time schedule (CfgD::P)
    (3000, 3000, 16, "dpss", {"NW": 4, "Kmax": 7}, "pow", False, 0, False),
    (2700, 3000, 7, "dpss", {"NW": 3, "Kmax": 5}, "fourier", True, 1, True),
    (6000, 6000, 8, "dpss", {"NW": 3, "Kmax": 3}, "fourier", False, 0, False),
    (7500, 7500, 5, "hann", {}, "abs", True, None, False),
    (1500, 1500, 9, "dpss", {"NW": 2, "Kmax": 3}, "pow", True, 0, True),
    (600, 600, 33, "hann", {}, "fourier", True, 0, False),
    (10000, 10000, 8, "dpss", {"NW": 3, "Kmax": 4}, "pow", False, 0, False),           # split exchanges, 20 values per thread
    (100, 100, 70, "hann", {}, "pow", True, 0, False),                                 # sliding-window lengths 10 x 10, 3 x 100
    (400, 400, 36, "hann", {}, "fourier", True, 0, False),                             # 20 values per thread: 400 ... 8000
    (1100, 1200, 10, "dpss", {"NW": 2, "Kmax": 3}, "pow", False, 1, True),
    (1600, 1600, 8, "dpss", {"NW": 3, "Kmax": 5}, "fourier", False, 0, False),
    (3200, 3200, 5, "dpss", {"NW": 2, "Kmax": 2}, "abs", True, None, False),
    (4800, 4800, 4, "dpss", {"NW": 2, "Kmax": 3}, "pow", False, 0, False),
    (8000, 8000, 7, "hann", {}, "fourier", True, 0, False),
    (280, 300, 33, "dpss", {"NW": 2, "Kmax": 3}, "fourier", True, 1, False),
    (768, 768, 12, "dpss", {"NW": 2, "Kmax": 3}, "fourier", True, 0, False),           # 3 x 256 ... 3 x 2048
    (1400, 1536, 6, "hann", {}, "pow", True, 1, False),
    (3072, 3072, 8, "dpss", {"NW": 4, "Kmax": 7}, "pow", False, 0, True),
    (6144, 6144, 5, "dpss", {"NW": 2, "Kmax": 2}, "fourier", False, 0, False),
    (9000, 10000, 5, "dpss", {"NW": 2, "Kmax": 2}, "fourier", True, 1, True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_N{c[1]}_C{c[2]}_{c[5]}" for c in CASES])
def test_fft_vs_oracle(be, case):
    nsig, nfft, C, taper, topt, output, keeptapers, detrend, dm = case
    rng = np.random.default_rng(nsig * 7 + C)
    starts = [5, 5 + nsig, 11 + 2 * nsig]
    data = rng.normal(size=(3 * nsig + 40, C)).astype(np.float32)
    got, plan = _run_fft(be, data, nsig, nfft, taper, topt, output, keeptapers, detrend, dm, None, None, starts)
    ref = _oracle_fft(data, starts, nsig, nfft, taper, topt, output, keeptapers, detrend, dm, None, None)
    # the angle of a near-zero bin is ill-conditioned: compare on the unit circle instead
    if output == "angle":
        got, ref = np.exp(1j * got), np.exp(1j * ref.astype(np.float64))
        assert np.abs(got - ref).max() < 2e-3
        return
    assert_parity(got, ref, what=plan.kernel_name)


@pytest.mark.parametrize("nsig,nfft", [(1024, 1024), (5000, 5000), (11000, 12000), (16384, 16384), (20000, 20000)])
def test_fft_freq_and_channel_selection(be, nsig, nfft):
    """Frequency and channel selections (repeated and reordered channels, an odd count) - also through the pair forms of the
    long-trial kernels, whose bins f and nfft/2 - f leave one thread together."""
    rng = np.random.default_rng(3)
    data = rng.normal(size=(3 * nsig + 200, 12)).astype(np.float32)
    fidx = np.array([7, 3, 100, nfft // 2, 0, nfft // 2 - 1, nfft // 4, nfft // 4 + 1, nfft // 4 - 1], dtype=np.int32)
    cidx = [11, 0, 5, 5, 2]
    starts = [0, 2 * nsig, 100]
    for output, keep in (("pow", False), ("fourier", True), ("real", True)):
        got, plan = _run_fft(be, data, nsig, nfft, "dpss", {"NW": 3, "Kmax": 5}, output, keep, 0, False, fidx, cidx,
                             starts)
        ref = _oracle_fft(data, starts, nsig, nfft, "dpss", {"NW": 3, "Kmax": 5}, output, keep, 0, False, fidx, cidx)
        assert_parity(got, ref, what=f"{plan.kernel_name} {output}")


def test_fft_zero_extended_segments_of_long_trials(be):
    """Segments of the pair-form kernels that stick out of [lo, hi) on either side, with an odd first row inside."""
    rng = np.random.default_rng(6)
    nsig = nfft = 12000
    data = rng.normal(size=(30000, 5)).astype(np.float32)
    starts = np.array([-3001, 0, 20001, 9000], dtype=np.int64)
    lo = np.array([0, 0, 15000, 9001], dtype=np.int64)
    hi = np.array([30000, 30000, 30000, 12346], dtype=np.int64)
    tapers = O.taper_table("hann", nsig, nfft)
    plan = be.FFTPlan(nsig, nfft, 5, tapers, O.spec_scale(nsig, nfft), None, False, None, "fourier", True)
    dev = torch.from_numpy(data).cuda()
    got = plan.execute(dev, torch.from_numpy(starts).cuda(), torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()).cpu().numpy()
    for b in range(len(starts)):
        x = np.zeros((nsig, 5), np.float32)
        a0, a1 = max(starts[b], lo[b]), min(starts[b] + nsig, hi[b])
        x[a0 - starts[b]:a1 - starts[b]] = data[a0:a1]
        ref, _ = O.mtmfft_cF(x, foi=np.fft.rfftfreq(nfft, 1e-3), keeptapers=True, polyremoval=None, output="fourier",
                             method_kwargs=dict(samplerate=1000.0, taper="hann", taper_opt={}, nSamples=nfft, demean_taper=False))
        assert_parity(got[b], ref[0], what=f"{plan.kernel_name} segment {b}")


def test_fft_zero_extended_segments(be):
    """Segments that stick out of [lo, hi) read zeros there (STFT boundary handling, stft.py:101-117)."""
    rng = np.random.default_rng(5)
    nsig = nfft = 512
    data = rng.normal(size=(3000, 6)).astype(np.float32)
    starts = np.array([-256, 0, 2744, 1000], dtype=np.int64)
    lo = np.array([0, 0, 1000, 1100], dtype=np.int64)
    hi = np.array([3000, 3000, 3000, 1300], dtype=np.int64)
    tapers = O.taper_table("hann", nsig, nfft)
    plan = be.FFTPlan(nsig, nfft, 6, tapers, np.sqrt(2) / nsig, 0, False, None, "fourier", True)
    d = torch.from_numpy(data).cuda()
    out = plan.execute(d, torch.from_numpy(starts).cuda(), torch.from_numpy(lo).cuda(),
                       torch.from_numpy(hi).cuda()).cpu().numpy()
    for b in range(4):
        seg = np.zeros((nsig, 6), np.float32)
        for n in range(nsig):
            r = starts[b] + n
            if lo[b] <= r < hi[b]:
                seg[n] = data[r]
        seg = seg - seg.mean(axis=0)
        ref = (np.fft.rfft(tapers[0][:, None] * seg, axis=0) * (np.sqrt(2) / nsig)).astype(np.complex64)
        assert_parity(out[b, 0], ref, what=f"segment {b}")


@pytest.mark.parametrize("C,N,B,K", [(256, 4096, 3, 2), (6, 512, 5, 3), (37, 1024, 4, 1), (8, 8192, 2, 2)])
def test_blocked_handover_layout_is_bit_identical(be, C, N, B, K):
    """FFT -> CSD through the channel-blocked hand-over layout (coalesced stores) gives the accumulator of the
    (B, K, F, C) path (bit for bit where both layouts run the same kernel), and the blocked spectra are a pure
    re-ordering of the standard ones."""
    rng = np.random.default_rng(C)
    data = torch.from_numpy(rng.normal(size=(B * N, C)).astype(np.float32)).cuda()
    starts = torch.arange(B, device="cuda", dtype=torch.int64) * N
    tapers = O.taper_table("dpss", N, N, {"NW": 2.0, "Kmax": K}) if K > 1 else O.taper_table("hann", N, N)
    F = N // 2 + 1
    mk = lambda: be.FFTPlan(N, N, C, tapers, np.sqrt(2) / N, 0, False, None, "fourier", True)   # noqa: E731
    p_std, p_blk = mk(), mk()
    assert p_blk.set_blocked(True)
    s_std = p_std.execute(data, starts)
    s_blk = p_blk.execute(data, starts)
    assert tuple(s_blk.shape) == (B * K, (C + 3) // 4, F, 4)
    got = s_blk.permute(0, 2, 1, 3).reshape(B * K, F, 4 * ((C + 3) // 4))     # back to (rows, F, padded channels)
    assert torch.equal(torch.view_as_real(got[:, :, :C].contiguous()),
                       torch.view_as_real(s_std.reshape(B * K, F, C)))
    if C % 4:
        assert float(got[:, :, C:].abs().max()) < 1e-5                        # padding channels: rounding residue only
    a_std = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    a_blk = torch.zeros_like(a_std)
    be.csd_accumulate(s_std, a_std)
    be.csd_accumulate(s_blk, a_blk, blocked=True)
    # what consumers read is the lower triangle (the rest of a diagonal tile is never looked at)
    be.csd_finalize(a_std, 1.0)
    be.csd_finalize(a_blk, 1.0)
    # the standard layout takes the 3-multiplication kernels (every channel count up to 512 since round 3), the blocked
    # one the 4-multiplication kernels (256 channels: the 3M kernel with gathering copies): same products, different
    # float32 addition order
    assert_parity(a_std.cpu().numpy(), a_blk.cpu().numpy(), what="blocked vs standard layout")
    with be.csd_phase_exact(True):             # the same kernel family on both layouts: bit-identical accumulators
        a4 = torch.zeros_like(a_std)
        be.csd_accumulate(s_std, a4)
        be.csd_finalize(a4, 1.0)
        if C != 256:
            assert torch.equal(torch.view_as_real(a4), torch.view_as_real(a_blk))
    assert not be.FFTPlan(N, N, C, tapers, np.sqrt(2) / N, 0, False, None, "pow", True).set_blocked(True)


@pytest.mark.parametrize("C,F", [(37, 9), (256, 3)])
def test_coh_from_accumulator_is_bit_identical(be, C, F):
    """Fused K5 (scale + normalise + convert + mirror from the raw lower-triangle accumulator) against
    csd_finalize + coh_normalize: same float operations, identical bits, accumulator untouched."""
    R = 40
    g = torch.Generator(device="cuda").manual_seed(C)
    spec = torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, device="cuda", dtype=torch.float32))
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    raw = acc.clone()
    fused = {o: be.coh_from_accumulator(acc, 1.0 / R, o) for o in ("abs", "pow", "complex", "imag", "real", "angle")}
    assert torch.equal(torch.view_as_real(acc), torch.view_as_real(raw))
    be.csd_finalize(acc, 1.0 / R)
    for o, got in fused.items():
        ref = be.coh_normalize(acc, o)
        a, b = (torch.view_as_real(got), torch.view_as_real(ref)) if got.is_complex() else (got, ref)
        assert torch.equal(a, b), o


def test_csd_tril_pack_roundtrip(be):
    """Packed lower triangle (what the multi-GPU all-reduce ships): pack -> unpack restores the lower triangle
    bit-exactly and leaves the upper one alone; the finalised CSD is unchanged."""
    C, F, R = 37, 9, 12
    g = torch.Generator(device="cuda").manual_seed(5)
    spec = torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, device="cuda", dtype=torch.float32))
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    packed = be.csd_tril_pack(acc)
    assert tuple(packed.shape) == (F, C * (C + 1) // 2)
    ii, jj = np.tril_indices(C)
    assert torch.equal(torch.view_as_real(packed), torch.view_as_real(acc[:, ii, jj].contiguous()))
    other = torch.full_like(acc, 7.0)
    be.csd_tril_unpack(packed, other)
    assert torch.equal(torch.view_as_real(other[:, ii, jj].contiguous()), torch.view_as_real(packed))
    iu, ju = np.triu_indices(C, 1)
    assert bool((other[:, iu, ju] == 7.0).all())
    ref = acc.clone()
    be.csd_finalize(ref, 1.0 / R)
    be.csd_finalize(other, 1.0 / R)
    assert torch.equal(torch.view_as_real(ref), torch.view_as_real(other))


def test_csd_tail_row_split(be):
    """259 workgroups on 256 CUs with enough rows that the re-cut tail is also split over rows (partial sums in
    library scratch + fixed-order reduction); reference = complex128 matrix products of the same spectra."""
    C, F, R = 256, 259, 300
    g = torch.Generator(device="cuda").manual_seed(3)
    spec = torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, device="cuda", dtype=torch.float32))
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec[:130].contiguous(), acc)
    be.csd_accumulate(spec[130:].contiguous(), acc)
    be.csd_finalize(acc, 1.0 / R)
    got = acc.cpu().numpy()
    for f in (0, 100, 255, 256, 257, 258):
        x = spec[:, f, :].to(torch.complex128)
        ref = (x.T @ x.conj() / R).cpu().numpy()
        assert_parity(got[f], ref.astype(np.complex64), what=f"csd f={f}")
    be.csd_accumulate(spec, acc)                      # same call again: results must be bit-identical (deterministic)
    a1 = acc.clone()
    acc.copy_(torch.from_numpy(got).cuda())
    be.csd_accumulate(spec, acc)
    assert torch.equal(torch.view_as_real(a1), torch.view_as_real(acc))


@pytest.mark.parametrize("C,F,R", [(5, 33, 14), (16, 101, 140), (40, 17, 35), (70, 9, 64), (256, 5, 70),
                                   (256, 259, 10),     # 259 workgroups on 256 CUs: exercises the re-cut tail
                                   (128, 131, 20), (64, 1027, 9), (192, 300, 12),   # lean path, several f per row
                                   # 3M kernel with generated sub-tile tables: partial last packed rows, its tail
                                   (160, 259, 10), (224, 6, 13), (96, 515, 9), (32, 2051, 5), (320, 131, 9), (384, 87, 10),
                                   (48, 1283, 9), (240, 258, 10),
                                   # every other multiple of 16 up to 512 (generated tables; NP = 2 ... 5 workgroups per
                                   # frequency above 256 channels)
                                   (16, 300, 12), (80, 200, 9), (112, 77, 10), (144, 130, 9), (176, 50, 12), (208, 33, 9),
                                   (272, 40, 9), (288, 9, 20), (304, 17, 9), (336, 12, 9), (352, 9, 9), (368, 8, 10),
                                   (400, 9, 9), (416, 7, 9), (432, 10, 9), (448, 10, 9), (464, 5, 12), (480, 9, 12), (496, 6, 9),
                                   (384, 7, 40), (512, 65, 20), (300, 130, 10),     # wide variant (+ its tail)
                                   (255, 270, 9), (63, 33, 14), (127, 3, 40), (301, 5, 12),    # odd channel counts
                                   # more than 512 channels: 3M products per 256-channel block + rectangle kernel
                                   (640, 5, 9), (768, 3, 10), (1024, 2, 9), (700, 4, 9), (513, 3, 9), (1025, 2, 5),
                                   (528, 70, 8)])
def test_csd_accumulate_vs_oracle(be, C, F, R):
    rng = np.random.default_rng(C + F)
    spec = (rng.normal(size=(R, F, C)) + 1j * rng.normal(size=(R, F, C))).astype(np.complex64)
    ref = np.einsum("rfi,rfj->fij", spec.astype(np.complex128), spec.conj().astype(np.complex128)) / R
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    s = torch.from_numpy(spec).cuda()
    half = R // 2
    be.csd_accumulate(s[:half].contiguous(), acc)      # two launches: accumulation across calls
    be.csd_accumulate(s[half:].contiguous(), acc)
    be.csd_finalize(acc, 1.0 / R)
    got = acc.cpu().numpy()
    assert_parity(got, ref.astype(np.complex64), what="csd")
    assert np.all(got.imag[:, np.arange(C), np.arange(C)] == 0)
    assert np.array_equal(got, np.conj(got.transpose(0, 2, 1)))
    for output in ("abs", "pow", "complex", "angle", "imag", "real"):
        coh = be.coh_normalize(acc, output).cpu().numpy()
        cref = O.normalize_csd(got, output)
        if output == "angle":
            assert np.abs(np.exp(1j * coh) - np.exp(1j * cref)).max() < 1e-4
        else:
            assert_parity(coh, cref, what=f"coh {output}")


@pytest.mark.parametrize("C,F,R", [(640, 3, 200), (513, 2, 101), (1030, 1, 64)])
def test_csd_phase_exact_more_than_512_channels(be, C, F, R):
    """spyhip_csd_set_phase_exact above 512 channels: the tiled kernel's 4-multiplication instances
    (csd3m_kernel<..., M4 = true>).  Channels that are real multiples of one signal plus a little noise: the imaginary
    part of every cross spectrum is tiny against its modulus, which the 3M product cannot resolve and this one does."""
    rng = np.random.default_rng(C)
    common = rng.normal(size=(R, F, 1)) + 1j * rng.normal(size=(R, F, 1))
    spec = (common * (1 + 0.1 * rng.normal(size=(1, 1, C))) + 1e-3 * (rng.normal(size=(R, F, C)) + 1j * rng.normal(size=(R, F, C)))).astype(np.complex64)
    ref = np.einsum("rfi,rfj->fij", spec.astype(np.complex128), spec.conj().astype(np.complex128))
    s = torch.from_numpy(spec).cuda()
    ii, jj = np.tril_indices(C, -1)
    err = {}
    for exact in (False, True):
        acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
        with be.csd_phase_exact(exact):
            be.csd_accumulate(s[: R // 2].contiguous(), acc)
            be.csd_accumulate(s[R // 2:].contiguous(), acc)
        got = acc.cpu().numpy()
        assert_parity(got[:, ii, jj], ref[:, ii, jj].astype(np.complex64), what=f"wide csd (phase exact {exact})")
        err[exact] = np.abs(got[:, ii, jj].imag - ref[:, ii, jj].imag).max() / np.abs(ref[:, ii, jj]).max()
    assert err[True] < 2e-7 and err[True] < 0.5 * err[False], err


@pytest.mark.parametrize("C,F,T,K", [(5, 33, 6, 3), (40, 17, 9, 1), (70, 9, 12, 7), (256, 3, 40, 7)])
def test_ppc_vs_oracle(be, C, F, T, K):
    """K7 (phasor sums + closed form) against the oracle's walk over all trial pairs; both entry points; accumulation
    across launches; an all-zero channel has ppc = 1 with everything (np.angle(0) = 0 in the reference)."""
    rng = np.random.default_rng(C + T)
    spec = (rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))).astype(np.complex64)
    spec += (2.0 * rng.normal(size=(1, K, F, C))).astype(np.complex64)          # common part: non-trivial consistency
    spec[..., C - 1] = 0
    st = O.spectral_dyadic_product(spec)                                       # (T, F, C, C) complex64
    ref = O.ppc(st)[0]
    s = torch.from_numpy(spec).cuda().reshape(T * K, F, C)
    U = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    half = (T // 2) * K
    be.ppc_accumulate(s[:half].contiguous(), K, U)
    be.ppc_accumulate(s[half:].contiguous(), K, U)
    got = be.ppc_finalize(U, T, lower_only=True).cpu().numpy()
    # the phase of a single-trial cross spectrum is only as good as |S| against the rounding of its K products
    assert_parity(got, ref, what="ppc", rtol=1e-4, atol_rel=2e-5)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    assert np.allclose(got[:, C - 1, :], 1, atol=1e-6) and np.allclose(got[:, np.arange(C), np.arange(C)], 1, atol=1e-6)
    U2 = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.ppc_accumulate_csd(torch.from_numpy(st).cuda(), U2)
    got2 = be.ppc_finalize(U2, T, lower_only=False).cpu().numpy()
    assert_parity(got2, ref, what="ppc from csd", rtol=1e-4, atol_rel=2e-5)


@pytest.mark.parametrize("C,N,T,pr", [(5, 700, 3, 0), (40, 1365, 2, 1), (70, 301, 4, None), (12, 4096, 2, 0),
                                      (33, 5461, 1, 0)])
def test_ccov_vs_oracle(be, C, N, T, pr):
    """K8 against the oracle's literal walk over channel pairs (even / odd N incl. the reference's one-lag-late upper
    triangle for even N, every transform length 1024..8192, all normalisations)."""
    import syncopy_amd.connectivity.ST_compRoutines as ST
    rng = np.random.default_rng(C + N)
    x = rng.normal(size=(T, N, C)).astype(np.float32)
    x[:, 1:] += 0.6 * x[:, :-1]
    x[:, 3:, 1] += 0.5 * x[:, :-3, 0]                       # a lagged coupling: asymmetric in the lag
    x += rng.normal(size=(1, 1, C)).astype(np.float32)      # channel offsets (matter for polyremoval=None)
    ref = np.mean([O.cross_covariance(t, 1.0, pr, False)[0] for t in x], axis=0)[:, 0]
    dev = torch.from_numpy(x.reshape(T * N, C)).cuda()
    rows = [(t * N, (t + 1) * N) for t in range(T)]
    acc, n = ST._ccov_trials(dev, rows, None, pr)
    got = be.ccov_from_accumulator(acc, N, 1.0 / T, 0).cpu().numpy()
    assert got.shape == ref.shape
    assert_parity(got, ref.astype(np.float32), what="ccov", atol_rel=1e-5)
    assert_parity(be.ccov_from_accumulator(acc, N, 1.0 / T, 1).cpu().numpy(),
                  O.normalize_ccov(ref[:, None])[:, 0].astype(np.float32), what="ccov normalised", atol_rel=1e-5)
    assert_parity(be.ccov_normalize_(torch.from_numpy(got).cuda()).cpu().numpy(),
                  O.normalize_ccov(ref[:, None])[:, 0].astype(np.float32), what="ccov_normalize", atol_rel=1e-5)
    acc1, _ = ST._ccov_trials(dev, rows[:1], None, pr)
    ref1 = O.cross_covariance(x[0], 1.0, pr, True)[0][:, 0]
    assert_parity(be.ccov_from_accumulator(acc1, N, 1.0, 2).cpu().numpy(), ref1.astype(np.float32),
                  what="single-trial cross-correlation (np.std products)", atol_rel=1e-5)


def test_slt_combine_and_convert(be):
    """One factor of the superlet geometric mean (principal-branch complex power, 0^e = 0, exponent 0 = untouched,
    scale offset, > 128 scales per call) and the real conversions, against NumPy."""
    rng = np.random.default_rng(8)
    nseg, nt, ns, nsub, s0, C = 2, 37, 150, 140, 10, 3
    acc = (rng.normal(size=(nseg, nt, ns, C)) + 1j * rng.normal(size=(nseg, nt, ns, C))).astype(np.complex64)
    spec = (rng.normal(size=(nseg, nt, nsub, C)) + 1j * rng.normal(size=(nseg, nt, nsub, C))).astype(np.complex64)
    spec[0, 0, 0, 0] = 0
    spec[0, 1, 1, 0] = -2.0                              # on the branch cut: arg = +pi
    expo = rng.uniform(0.1, 1.0, size=nsub)
    expo[5] = 0.0
    ref = acc.astype(np.complex128)
    ref[:, :, s0:] *= np.power(spec.astype(np.complex128).transpose(0, 1, 3, 2), expo).transpose(0, 1, 3, 2)
    d_acc, d_spec = torch.from_numpy(acc).cuda(), torch.from_numpy(spec).cuda()
    got = be.slt_combine(d_acc, d_spec, s0, expo, init=False).cpu().numpy()
    assert_parity(got, ref.astype(np.complex64), what="slt_combine")
    assert np.array_equal(got[:, :, :s0], acc[:, :, :s0]) and np.array_equal(got[:, :, s0 + 5], acc[:, :, s0 + 5])
    init = be.slt_combine(torch.from_numpy(acc).cuda(), d_spec, s0, expo, init=True).cpu().numpy()
    want = np.power(spec.astype(np.complex128).transpose(0, 1, 3, 2), expo).transpose(0, 1, 3, 2)
    assert_parity(init[:, :, s0:], want.astype(np.complex64), what="slt_combine init")
    assert init[0, 0, s0, 0] == 0 and np.all(init[:, :, s0 + 5] == 1)
    mod = be.slt_combine(torch.from_numpy(np.abs(acc).astype(np.complex64)).cuda(), d_spec, s0, expo, init=False,
                         modulus_only=True).cpu().numpy()
    assert_parity(mod.real[:, :, s0:], np.abs(ref[:, :, s0:]).astype(np.float32), what="slt_combine modulus")
    assert np.all(mod.imag == 0)
    racc = torch.from_numpy(np.abs(acc)).cuda()
    rspec = torch.from_numpy(np.abs(spec)).cuda()
    rgot = be.slt_combine(racc.clone(), rspec, s0, expo, init=False).cpu().numpy()
    assert_parity(rgot[:, :, s0:], np.abs(ref[:, :, s0:]).astype(np.float32), what="slt_combine real")
    rsq = be.slt_combine(racc.clone(), rspec, s0, expo, init=False, square=True).cpu().numpy()
    assert_parity(rsq[:, :, s0:], (np.abs(ref[:, :, s0:]) ** 2).astype(np.float32), what="slt_combine real squared")
    assert np.array_equal(rsq[:, :, :s0], np.abs(acc)[:, :, :s0])
    for kind, fn in (("pow", lambda z: np.abs(z) ** 2), ("abs", np.abs), ("real", np.real), ("imag", np.imag)):
        assert_parity(be.spec_convert(d_spec, kind).cpu().numpy(), fn(spec.astype(np.complex128)).astype(np.float32),
                      what=kind)
    assert be.spec_convert(d_spec, "fourier") is d_spec


def test_cwt_trial_sum_mode(be):
    """accumulate=2 (out[0] += sum over segments, the keeptrials=False path) equals the sum of the per-segment
    outputs of the plain mode; 5 channels exercise the padded channel pair of the packed kernel."""
    rng = np.random.default_rng(11)
    nsig, C, T = 700, 5, 7
    data = torch.from_numpy(rng.normal(size=(T * nsig, C)).astype(np.float32)).cuda()
    scales = (1 / np.array([10., 25., 60.])) * (6 + np.sqrt(38)) / (4 * np.pi)
    plan = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, "pow")
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig
    each = plan.execute(data, st, st, st + nsig)
    total = torch.zeros(plan.out_shape(1), dtype=torch.float32, device="cuda")
    plan.execute(data, st[:4].contiguous(), st[:4].contiguous(), (st[:4] + nsig).contiguous(), out=total, accumulate=2)
    plan.execute(data, st[4:].contiguous(), st[4:].contiguous(), (st[4:] + nsig).contiguous(), out=total, accumulate=2)
    ref = each.double().sum(dim=0, keepdim=True).float()
    assert_parity(total.cpu().numpy(), ref.cpu().numpy(), what="cwt trial sum")


def test_cwt_wide_transposition_tiles(be):
    """Real outputs of trials of >= 1024 samples leave the staging buffer through 256-sample x 16-channel tiles
    (cwt_scatter_wide_kernel): ragged in both directions (1500 samples, 21 channels), every accumulation mode and a
    post-selection of samples, against the oracle."""
    rng = np.random.default_rng(13)
    nsig, C, T = 1500, 21, 5
    x = rng.normal(size=(T * nsig, C)).astype(np.float32)
    freqs = np.array([12.0, 30.0, 70.0])
    scales = (1 / freqs) * (6 + np.sqrt(38)) / (4 * np.pi)
    data = torch.from_numpy(x).cuda()
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig
    ref = np.stack([O.convert_output(O.cwt(O.detrend(x[t * nsig:(t + 1) * nsig], 0), 1000.0, scales).transpose(1, 0, 2), "pow")
                    for t in range(T)])
    plan = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, "pow")
    each = plan.execute(data, st, st, st + nsig)
    assert_parity(each.cpu().numpy(), ref, what="wide tiles, per segment")
    total = torch.zeros(plan.out_shape(1), dtype=torch.float32, device="cuda")
    plan.execute(data, st[:2].contiguous(), st[:2].contiguous(), (st[:2] + nsig).contiguous(), out=total, accumulate=2)
    plan.execute(data, st[2:].contiguous(), st[2:].contiguous(), (st[2:] + nsig).contiguous(), out=total, accumulate=2)
    assert_parity(total.cpu().numpy()[0], ref.astype(np.float64).sum(axis=0).astype(np.float32), what="wide tiles, trial sum")
    acc = each.clone()
    plan.execute(data, st, st, st + nsig, out=acc, accumulate=True)
    assert_parity(acc.cpu().numpy(), 2 * ref, what="wide tiles, out[b] += segment b")
    keep = np.r_[3:700:7, 1023, 1024, 1499]                      # post-selection: output slot of sample n, or -1
    tpos = np.full(nsig, -1, dtype=np.int32)
    tpos[keep] = np.arange(keep.size)
    sel = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, "pow", tpos=tpos, ntime_out=keep.size)
    got = sel.execute(data, st, st, st + nsig)
    assert_parity(got.cpu().numpy(), ref[:, keep], what="wide tiles, selected samples")


@pytest.mark.parametrize("output", ["pow", "abs", "fourier"])
@pytest.mark.parametrize("C", [21, 32, 1])
def test_cwt_direct_kernels_equal_the_staged_path(be, output, C):
    """cwt2d_kernel (1024- / 2048-point blocks written in the output layout by the transform kernel) against the same plan
    with every scale through the staging buffer and the transposition pass (set_direct(False)): the same arithmetic per
    value up to the compiler's contraction choices (agreement to 2e-6, five times tighter than the parity criterion); trial
    sums differ in summation order as well.  Scales
    on several block lengths at once (45, 70, 95 Hz: 1024 points, 30 Hz: 2048, 8 Hz: 1211 taps on 8192-point blocks - staged
    in either mode), odd channel counts (the padded pair and the unaligned scalar stores), a post-selection of samples."""
    rng = np.random.default_rng(17)
    nsig, T = 3000, 5
    x = rng.normal(size=(T * nsig, C)).astype(np.float32) + 3.0
    freqs = np.array([8.0, 30.0, 45.0, 70.0, 95.0])
    scales = (1 / freqs) * (6 + np.sqrt(38)) / (4 * np.pi)
    data = torch.from_numpy(x).cuda()
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig
    keep = np.r_[0:5, 3:2900:7, 1023, 1024, 2047, 2048, 2999]
    keep = np.unique(keep)
    tpos = np.full(nsig, -1, dtype=np.int32)
    tpos[keep] = np.arange(keep.size)
    for kw in ({}, {"tpos": tpos, "ntime_out": keep.size}):
        direct = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, output, **kw)
        staged = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, output, **kw)
        staged.set_direct(False)
        a = direct.execute(data, st, st, st + nsig)
        b = staged.execute(data, st, st, st + nsig)
        # (two instantiations of the same engine: the compiler contracts multiply-adds differently, so not bit for bit)
        assert_parity(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-6, atol_rel=2e-7, what=f"direct vs staged, {output}, {C} ch, tpos={bool(kw)}")
        a2, b2 = a.clone(), b.clone()
        direct.execute(data, st, st, st + nsig, out=a2, accumulate=True)
        staged.execute(data, st, st, st + nsig, out=b2, accumulate=True)
        assert_parity(a2.cpu().numpy(), b2.cpu().numpy(), rtol=2e-6, atol_rel=2e-7, what="direct vs staged, out[b] += segment b")
        assert_parity(a2.cpu().numpy(), 2 * a.cpu().numpy(), rtol=1e-6, atol_rel=1e-7, what="direct, out[b] += segment b")
        ta = torch.zeros(direct.out_shape(1), dtype=a.dtype, device="cuda")
        tb = torch.zeros(direct.out_shape(1), dtype=a.dtype, device="cuda")
        for lo, hi in ((0, 2), (2, 5)):
            direct.execute(data, st[lo:hi].contiguous(), st[lo:hi].contiguous(), (st[lo:hi] + nsig).contiguous(), out=ta, accumulate=2)
            staged.execute(data, st[lo:hi].contiguous(), st[lo:hi].contiguous(), (st[lo:hi] + nsig).contiguous(), out=tb, accumulate=2)
        ref = (a.to(torch.complex128) if a.is_complex() else a.double()).sum(dim=0, keepdim=True)
        assert_parity(ta.cpu().numpy(), ref.cpu().numpy().astype(ta.cpu().numpy().dtype), what="direct trial sum")
        assert_parity(tb.cpu().numpy(), ref.cpu().numpy().astype(tb.cpu().numpy().dtype), what="staged trial sum")


def test_cwt_trial_sums_long_signals_own_block_groups(be):
    """Trial sums of signals of 4096 samples and more run on their own block groups (at least 4096 points per block,
    cwt_route.h: Plan::groups_sum) with one channel of TWO trials per packed thread: 128 channels x 4500 samples x 37
    trials (an odd count: the last pair is half empty) in two calls, against the float64 sum of the per-trial outputs,
    which come from the 1024- / 2048-point direct kernels."""
    rng = np.random.default_rng(19)
    nsig, C, T = 4500, 128, 37
    data = torch.from_numpy(rng.normal(size=(T * nsig, C)).astype(np.float32)).cuda()
    scales = (1 / np.array([24.0, 40.0, 64.0, 100.0])) * (6 + np.sqrt(38)) / (4 * np.pi)
    plan = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, "pow")
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig
    total = torch.zeros(plan.out_shape(1), dtype=torch.float32, device="cuda")
    ref = torch.zeros(plan.out_shape(1), dtype=torch.float64, device="cuda")
    for lo, hi in ((0, 30), (30, 37)):
        s = st[lo:hi].contiguous()
        plan.execute(data, s, s, s + nsig, out=total, accumulate=2)
        ref += plan.execute(data, s, s, s + nsig).double().sum(dim=0, keepdim=True)
    assert_parity(total.cpu().numpy(), ref.float().cpu().numpy(), what="direct trial sum, 37 trials")


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_cwt_kernels_longer_than_one_block(be, output):
    """Morlet kernels of more than 8191 taps (transform.py:96-103 samples 10 s / dt of them and convolves in full,
    whatever the signal length): the plan cuts them into pieces of 8192 taps, every piece is its own overlap-save
    convolution on 16384-point blocks and the complex results add up before the output conversion.  20000 samples
    at 1 kHz: 0.3 Hz -> 32210 taps (4 pieces), 0.5 Hz -> 19326 (3), 1.5 Hz -> 6442 (one 16384-point block),
    20 Hz -> 483 (2048-point blocks); 3 channels exercise the padded pair of the packed kernel."""
    rng = np.random.default_rng(5)
    nsig, C, T = 20000, 3, 2
    x = (rng.normal(size=(T * nsig, C)) + np.sin(2 * np.pi * 0.4e-3 * np.arange(T * nsig))[:, None]).astype(np.float32)
    freqs = np.array([0.3, 0.5, 1.5, 20.0])
    scales = (1 / freqs) * (6 + np.sqrt(38)) / (4 * np.pi)
    plan = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, output)
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig
    got = plan.execute(torch.from_numpy(x).cuda(), st, st, st + nsig).cpu().numpy()
    for t in range(T):
        trl = O.detrend(x[t * nsig:(t + 1) * nsig], 0)
        ref = O.convert_output(O.cwt(trl, 1000.0, scales).transpose(1, 0, 2), output)
        assert_parity(got[t], ref, what=f"long cwt kernels, {output}, trial {t}")


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_cwt_trial_sum_of_a_plan_with_long_kernels(be, output):
    """A trial sum whose plan holds a 16384-point group and a scale in pieces (4500 samples: 0.9 Hz -> 8999 taps, pieces of
    8192 + 807; 1.6 Hz -> 6051 taps on 16384-point blocks; 20 Hz -> 2048-point blocks): the 16384-point kernel carries no
    pairs of trials, so the sum runs unpaired on the per-segment groups, every scale staged.  3 trials in calls of 2 and 1,
    against the float64 sum of the per-trial outputs."""
    rng = np.random.default_rng(23)
    nsig, C, T = 4500, 3, 3
    data = torch.from_numpy(rng.normal(size=(T * nsig, C)).astype(np.float32) + 0.5).cuda()
    scales = (1 / np.array([0.9, 1.6, 20.0])) * (6 + np.sqrt(38)) / (4 * np.pi)
    plan = be.CWTPlan(nsig, C, scales, 1e-3, 6.0, 0, output)
    st = torch.arange(T, device="cuda", dtype=torch.int64) * nsig
    total = torch.zeros(plan.out_shape(1), dtype=torch.complex64 if output == "fourier" else torch.float32, device="cuda")
    for lo, hi in ((0, 2), (2, 3)):
        s = st[lo:hi].contiguous()
        plan.execute(data, s, s, s + nsig, out=total, accumulate=2)
    each = plan.execute(data, st, st, st + nsig)
    ref = (each.to(torch.complex128) if each.is_complex() else each.double()).sum(dim=0, keepdim=True)
    assert_parity(total.cpu().numpy(), ref.cpu().numpy().astype(total.cpu().numpy().dtype), what=f"trial sum with long kernels, {output}")


def test_blocked_tail_starts_inside_a_frequency(be):
    """the (5,4) path of the blocked hand-over layout cuts work into 36-tile items whatever ntiles is, so
    the re-cut tail can start in the middle of a frequency (C = 192: 21 tiles).  The row-split reduction only covers
    whole frequencies - such tails must run unsplit.  The library scratch is dirtied first by a launch that does
    split (C = 256)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    spec = torch.view_as_complex(torch.randn((300, 259, 256, 2), generator=g, device="cuda"))
    acc = torch.zeros((259, 256, 256), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)                                  # leaves partial sums in ctx->scratch
    del spec, acc
    C, F, R = 192, 1001, 128
    spec = torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, device="cuda"))
    blk = spec.reshape(R, F, C // 4, 4).permute(0, 2, 1, 3).contiguous()
    a_std = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    a_blk = torch.zeros_like(a_std)
    be.csd_accumulate(spec, a_std)
    be.csd_accumulate(blk, a_blk, blocked=True)
    be.csd_finalize(a_std, 1.0 / R)
    be.csd_finalize(a_blk, 1.0 / R)
    assert_parity(a_blk.cpu().numpy(), a_std.cpu().numpy(), what="blocked tail")
    for f in (0, 500, 989, 990, 991, 1000):
        x = spec[:, f, :].to(torch.complex128)
        ref = (x.T @ x.conj() / R).cpu().numpy()
        assert_parity(a_blk[f].cpu().numpy(), ref.astype(np.complex64), what=f"blocked csd f={f}")


# ---------------------------------------------------------------------------------------------------------------
# K1 at the reference's precision (spyhip_fft_plan_set_precision): float64 taper product + FFT, complex64 rounding
def _harmonic_fixture(N=4096):
    """Harmonics + a noise floor 60 dB below them (tools/precision_report.py): the dynamic range the float32 transform
    cannot resolve bin by bin."""
    t = np.arange(N) / 1000.0
    rng = np.random.default_rng(0)
    harm = np.stack([np.cos(2 * np.pi * f * t) for f in (40.0, 100.0, 7.3, 333.0)], axis=1)
    return (harm + 1e-3 * rng.normal(size=harm.shape)).astype(np.float32)


def test_reference_precision_resolves_60dB(be):
    x = _harmonic_fixture()
    N, C = x.shape
    tap = O.taper_table("hann", N, N, {})
    sc = O.spec_scale(N, N)
    ref, _ = O.mtmfft(O.detrend(x.copy(), 0), 1000.0, N, "hann", {})
    ref = ref.astype(np.complex128)
    dev = torch.from_numpy(x).cuda()
    starts = torch.zeros(1, dtype=torch.int64, device="cuda")
    frac = {}
    for prec in ("float32", "reference"):
        plan = be.FFTPlan(N, N, C, tap, sc, 0, False, None, "fourier", True, reference_mean=True)
        if prec == "reference":
            assert plan.set_precision(True) and "64_kernel" in plan.kernel_name
        got = plan.execute(dev, starts).cpu().numpy()[0].astype(np.complex128)
        err = np.abs(got - ref)
        frac[prec] = float((err <= 1e-5 * np.abs(ref)).mean())
        assert_parity(got.astype(np.complex64), ref.astype(np.complex64), what=prec)
    print(f"bins within PURE rtol 1e-5 of the float64 reference: float32 {100 * frac['float32']:.1f} %, "
          f"reference precision {100 * frac['reference']:.2f} %")
    assert frac["reference"] >= 0.99 and frac["float32"] < 0.5


@pytest.mark.parametrize("case", [dict(nsig=4096, nfft=4096, K=7, output="pow", keeptapers=False, detrend=0, nchan=5),
                                  dict(nsig=700, nfft=1024, K=3, output="fourier", keeptapers=True, detrend=1, nchan=4),
                                  dict(nsig=256, nfft=256, K=2, output="abs", keeptapers=True, detrend=-1, nchan=3,
                                       demean=True),
                                  dict(nsig=2048, nfft=2048, K=4, output="fourier", keeptapers=False, detrend=0, nchan=2,
                                       freq_idx=[0, 5, 1024, 77]),
                                  # any other length: the generic Stockham kernel on work arrays in global memory
                                  dict(nsig=2000, nfft=2000, K=7, output="pow", keeptapers=False, detrend=0, nchan=5),
                                  dict(nsig=5000, nfft=5000, K=3, output="fourier", keeptapers=True, detrend=1, nchan=3),
                                  dict(nsig=1001, nfft=1001, K=2, output="abs", keeptapers=True, detrend=-1, nchan=2,
                                       demean=True),                                   # odd: 7 x 11 x 13
                                  dict(nsig=3000, nfft=4500, K=3, output="fourier", keeptapers=False, detrend=0, nchan=4,
                                       freq_idx=[0, 9, 2250, 300]),
                                  dict(nsig=10000, nfft=16384, K=2, output="pow", keeptapers=True, detrend=0, nchan=3),
                                  dict(nsig=100, nfft=100, K=2, output="fourier", keeptapers=True, detrend=0, nchan=1),
                                  # 3 x a scheduled length: radix-3 decimation in front of the schedule (CfgD64::P)
                                  dict(nsig=3000, nfft=3000, K=7, output="pow", keeptapers=False, detrend=0, nchan=5),
                                  dict(nsig=5500, nfft=6000, K=3, output="abs", keeptapers=True, detrend=1, nchan=3),
                                  dict(nsig=6144, nfft=6144, K=2, output="fourier", keeptapers=False, detrend=0, nchan=4,
                                       freq_idx=[0, 9, 3072, 300, 2048, 2049]),
                                  dict(nsig=1500, nfft=1500, K=2, output="abs", keeptapers=True, detrend=-1, nchan=7,
                                       demean=True),
                                  dict(nsig=7500, nfft=7500, K=2, output="fourier", keeptapers=True, detrend=0, nchan=2),
                                  dict(nsig=700, nfft=768, K=3, output="fourier", keeptapers=True, detrend=0, nchan=9),
                                  dict(nsig=600, nfft=600, K=2, output="pow", keeptapers=True, detrend=0, nchan=17),
                                  dict(nsig=1536, nfft=1536, K=2, output="fourier", keeptapers=True, detrend=0, nchan=5),
                                  dict(nsig=3072, nfft=3072, K=4, output="real", keeptapers=False, detrend=0, nchan=3),
                                  # sliding-window lengths and the other multiples of 100 (20 values per thread)
                                  dict(nsig=100, nfft=100, K=2, output="fourier", keeptapers=True, detrend=0, nchan=37),
                                  dict(nsig=300, nfft=300, K=2, output="pow", keeptapers=False, detrend=0, nchan=18),
                                  dict(nsig=350, nfft=400, K=3, output="abs", keeptapers=True, detrend=1, nchan=9),
                                  dict(nsig=800, nfft=800, K=2, output="abs", keeptapers=True, detrend=-1, nchan=5, demean=True),
                                  dict(nsig=1200, nfft=1200, K=2, output="fourier", keeptapers=True, detrend=0, nchan=6),
                                  dict(nsig=1600, nfft=1600, K=4, output="pow", keeptapers=False, detrend=0, nchan=4),
                                  dict(nsig=2400, nfft=2400, K=2, output="fourier", keeptapers=False, detrend=0, nchan=3,
                                       freq_idx=[0, 7, 1200, 800, 801]),
                                  dict(nsig=3200, nfft=3200, K=3, output="fourier", keeptapers=True, detrend=0, nchan=3),
                                  dict(nsig=4800, nfft=4800, K=2, output="pow", keeptapers=True, detrend=0, nchan=2),
                                  dict(nsig=8000, nfft=8000, K=2, output="fourier", keeptapers=True, detrend=0, nchan=3),
                                  # 10240 < N <= 20480: single channels through the schedule of N / 2 (CfgD64::HALF);
                                  # beyond that N = P M through HBM (mtmfft_declong64.h: 24000, 30000)
                                  dict(nsig=12000, nfft=12000, K=3, output="fourier", keeptapers=True, detrend=0, nchan=5),
                                  dict(nsig=15000, nfft=15000, K=3, output="pow", keeptapers=False, detrend=1, nchan=4),
                                  dict(nsig=14000, nfft=16000, K=2, output="fourier", keeptapers=False, detrend=0, nchan=3,
                                       freq_idx=[0, 5, 7998, 2000, 2001, 7999]),      # (bins M q: the k = 0 thread)
                                  dict(nsig=20000, nfft=20000, K=2, output="abs", keeptapers=True, detrend=-1, nchan=3,
                                       demean=True),
                                  dict(nsig=12288, nfft=12288, K=2, output="fourier", keeptapers=True, detrend=0, nchan=2),
                                  dict(nsig=24000, nfft=24000, K=2, output="fourier", keeptapers=True, detrend=0, nchan=2),
                                  dict(nsig=30000, nfft=30000, K=2, output="pow", keeptapers=False, detrend=1, nchan=3),
                                  dict(nsig=11999, nfft=12000, K=2, output="pow", keeptapers=True, detrend=1, nchan=3, demean=True),
                                  dict(nsig=16001, nfft=16384, K=2, output="fourier", keeptapers=True, detrend=0, nchan=1),
                                  dict(nsig=16384, nfft=16384, K=3, output="abs", keeptapers=False, detrend=0, nchan=3),
                                  dict(nsig=50000, nfft=50000, K=1, output="fourier", keeptapers=True, detrend=-1, nchan=1)])
def test_reference_precision_options(be, case):
    """Every option of the plan through the float64 kernel: padding, detrending modes, demean_taper, taper mean,
    conversions, frequency selection, odd channel counts - vs the oracle, which now agrees to complex64 rounding."""
    rng = np.random.default_rng(3)
    nsig, nfft, K, C = case["nsig"], case["nfft"], case["K"], case["nchan"]
    # offsets only where the reference's own float32 detrending is reproduced exactly (the sequential mean, K0); its
    # float32 least-squares line (scipy.signal.detrend -> LAPACK sgelsd) leaves ~1e-7 x offset of its own noise next to DC
    x = (rng.normal(size=(nsig + 7, C)) + np.arange(C) * (10.0 if case["detrend"] == 0 else 0.0)).astype(np.float32)
    taper, topt = ("dpss", {"NW": (K + 1) / 2, "Kmax": K})
    tap = O.taper_table(taper, nsig, nfft, topt)
    fi = case.get("freq_idx")
    plan = be.FFTPlan(nsig, nfft, C, tap, O.spec_scale(nsig, nfft), None if case["detrend"] < 0 else case["detrend"],
                      case.get("demean", False), fi, case["output"], case["keeptapers"], reference_mean=case["detrend"] == 0)
    assert plan.set_precision(True)
    got = plan.execute(torch.from_numpy(x).cuda(), torch.tensor([3], dtype=torch.int64, device="cuda")).cpu().numpy()[0]
    freqs = np.fft.rfftfreq(nfft, 1e-3)
    ref, _ = O.mtmfft_cF(np.array(x[3:3 + nsig]), foi=freqs if fi is None else freqs[fi], keeptapers=case["keeptapers"],
                         polyremoval=None if case["detrend"] < 0 else case["detrend"], output=case["output"],
                         method_kwargs=dict(samplerate=1000.0, taper=taper, taper_opt=topt, nSamples=nfft,
                                            demean_taper=case.get("demean", False)))
    assert_parity(got, ref[0], what=str(case))
    if case["output"] == "fourier":
        # bin by bin to complex64 rounding (the float32 scale multiplies rounded values on both sides)
        err = np.abs(got.astype(np.complex128) - ref[0])
        # (the line fit: the reference's own float32 lstsq noise; a taper mean adds K - 1 float32 additions and a division)
        rt = 1e-5 if case["detrend"] == 1 else (4e-7 if case["keeptapers"] else 1e-6)
        assert np.all(err <= rt * np.abs(ref[0]) + 1e-12 * np.abs(ref[0]).max()), float((err / np.abs(ref[0])).max())


def test_reference_precision_through_freqanalysis():
    import syncopy_amd as spy
    from syncopy_amd.shared.errors import SPYValueError
    x = _harmonic_fixture()
    data = spy.AnalogData(x, samplerate=1000.0)
    a = spy.freqanalysis(data, method="mtmfft", taper="hann", output="fourier", precision="reference")
    ref, _ = O.mtmfft(O.detrend(x.copy(), 0), 1000.0, 4096, "hann", {})
    err = np.abs(a.data[0].astype(np.complex128) - ref)
    assert (err <= 1e-5 * np.abs(ref)).mean() >= 0.99
    # 2000 samples: a decimal schedule; 4099 is prime: the float64 kernel in its Bluestein form (round 4: any length)
    b = spy.freqanalysis(spy.AnalogData(x[:2000], samplerate=1000.0), method="mtmfft", taper="hann", output="fourier",
                         precision="reference")
    ref, _ = O.mtmfft(O.detrend(x[:2000].copy(), 0), 1000.0, 2000, "hann", {})
    err = np.abs(b.data[0].astype(np.complex128) - ref)
    assert (err <= 1e-5 * np.abs(ref)).mean() >= 0.99
    xp = np.tile(x, (2, 1))[:4099]
    c = spy.freqanalysis(spy.AnalogData(xp, samplerate=1000.0), method="mtmfft", taper="hann", output="fourier",
                         precision="reference")
    ref, _ = O.mtmfft(O.detrend(xp.copy(), 0), 1000.0, 4099, "hann", {})
    err = np.abs(c.data[0].astype(np.complex128) - ref)
    assert (err <= 1e-5 * np.abs(ref)).mean() >= 0.99
    # the default ("auto") transforms complex outputs in float64 on the batched route, power spectra in float32
    d = spy.freqanalysis(data, method="mtmfft", taper="hann", output="fourier")
    assert np.array_equal(d.data, a.data)
    with pytest.raises(SPYValueError):
        spy.freqanalysis(data, method="mtmfft", precision="double")


@pytest.mark.parametrize("nsamp", [2048, 2000])
def test_reference_precision_through_connectivityanalysis(nsamp):
    """Coherence is a ratio of spectra: with a line 60 dB above the noise floor in every channel the float32
    transform's absolute error (5e-7 of the rms bin, i.e. of the line) is ~1e-3 of the noise bins the coherence away
    from the line is made of - outside the criterion; precision="reference" (float64 transform, complex64 rounding
    where mtmfft.py:104-127 rounds) is inside it."""
    import syncopy_amd as spy
    from oracle_routines import ORACLE_CONN
    from parity import excess
    rng = np.random.default_rng(3)
    ntr, nchan = 12, 6              # (2048: the radix-16 float64 kernel; 2000: the any-length one)
    t = np.arange(nsamp * ntr) / 1000.0
    x = rng.normal(size=(nsamp * ntr, nchan)) + 1000.0 * np.sin(2 * np.pi * 50.0 * t)[:, None] * rng.uniform(0.5, 1.5, size=nchan)
    trl = np.stack([np.arange(ntr) * nsamp, np.arange(1, ntr + 1) * nsamp, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=1000.0, trialdefinition=trl)
    kw = dict(method="coh", taper="hann", output="abs")
    ref = spy.connectivityanalysis(data, compute_method="sequential", routine_classes=ORACLE_CONN, **kw)
    fast = spy.connectivityanalysis(data, precision="float32", **kw)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        exact = spy.connectivityanalysis(data, precision="reference", **kw)
        auto = spy.connectivityanalysis(data, **kw)          # the default: looks at 16 trials' spectra, picks float64
        seq = spy.connectivityanalysis(data, compute_method="sequential", **kw)   # per-trial route: float64 by default
    assert np.array_equal(auto.data, exact.data)
    assert excess(seq.data, ref.data) <= 1.0
    # ppc: phases of single-trial cross spectra - the same data, the same switch
    pk = dict(method="ppc", taper="hann")
    pref = spy.connectivityanalysis(data, compute_method="sequential", routine_classes=ORACLE_CONN, **pk)
    e32 = excess(spy.connectivityanalysis(data, precision="float32", **pk).data, pref.data, atol_rel=5e-6)
    eauto = excess(spy.connectivityanalysis(data, **pk).data, pref.data, atol_rel=5e-6)
    print(f"ppc away from a 60 dB line: float32 err/tol {e32:.3g}, precision='auto' {eauto:.3g}")
    assert eauto <= 1.0 < e32
    e_fast, e_exact = excess(fast.data, ref.data), excess(exact.data, ref.data)
    print(f"coherence away from a 60 dB line: float32 err/tol {e_fast:.3g}, precision='reference' {e_exact:.3g}")
    assert e_exact <= 1.0, e_exact
    assert e_fast > e_exact
    # 3001 samples: a prime - served by the Bluestein form of the float64 kernel since round 4
    refp = spy.connectivityanalysis(data, compute_method="sequential", routine_classes=ORACLE_CONN, pad=3.001, **kw)
    gotp = spy.connectivityanalysis(data, precision="reference", pad=3.001, **kw)
    assert excess(gotp.data, refp.data) <= 1.0


def test_auto_precision_for_granger():
    """precision="auto" for Granger causality: random-walk channels (1/f^2 spectra: the upper half of the axis sits
    60 dB and more below a channel's mean power) with a lagged coupling ask for float64 transforms - the default equals
    precision="reference", differs from "float32", and agrees with the oracle at the fuzz test's Granger tolerance."""
    import syncopy_amd as spy
    from oracle_routines import ORACLE_CONN
    rng = np.random.default_rng(11)
    nsamp, ntr, nchan = 1024, 40, 3
    e = rng.normal(size=(ntr, nsamp, nchan))
    w = np.cumsum(e, axis=1) + 0.05 * rng.normal(size=e.shape)
    w[:, 2:, 1] += 0.4 * w[:, :-2, 0]                                   # channel 0 drives channel 1
    x = w.reshape(ntr * nsamp, nchan).astype(np.float32)
    trl = np.stack([np.arange(ntr) * nsamp, np.arange(1, ntr + 1) * nsamp, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x, samplerate=1000.0, trialdefinition=trl)
    gk = dict(method="granger", taper="hann")           # 40 products: float64 from a dynamic range of 160 on
    gref = spy.connectivityanalysis(data, compute_method="sequential", routine_classes=ORACLE_CONN, **gk)
    gauto = spy.connectivityanalysis(data, **gk)
    gexact = spy.connectivityanalysis(data, precision="reference", **gk)
    g32 = spy.connectivityanalysis(data, precision="float32", **gk)
    assert np.array_equal(gauto.data, gexact.data) and not np.array_equal(gauto.data, g32.data)
    assert gauto.info["reg. factor"] == gref.info["reg. factor"]
    if gref.info["reg. factor"] != -1:
        np.testing.assert_allclose(gauto.data[:, 2:], gref.data[:, 2:], rtol=2e-3, atol=1e-2)


@pytest.mark.parametrize("method,kw", [("mtmconvol", dict(t_ftimwin=0.5, toi=0.5, taper="hann")),
                                       ("mtmconvol", dict(t_ftimwin=0.256, toi=0.75, tapsmofrq=8, polyremoval=1)),
                                       ("mtmconvol", dict(t_ftimwin=0.05, toi=np.arange(0.5, 1.5, 0.01), taper="hann")),
                                       ("welch", dict(t_ftimwin=0.4, toi=0.25, taper="hann"))])
def test_reference_precision_of_sliding_windows(method, kw):
    """precision="reference" for the sliding-window methods: 500- / 256- / 400-sample windows (the float64 any-length
    and register kernels on STFT frames) on data with a 60 dB line - inside the criterion, and bin by bin within pure
    rtol 1e-5 on at least 99 % of the bins."""
    import syncopy_amd as spy
    from oracle_routines import ORACLE_FREQ
    rng = np.random.default_rng(8)
    nsamp, ntr, nchan = 2000, 3, 4
    t = np.arange(nsamp * ntr) / 1000.0
    x = rng.normal(size=(nsamp * ntr, nchan)) + 1000.0 * np.sin(2 * np.pi * 50.0 * t)[:, None]
    trl = np.stack([np.arange(ntr) * nsamp, np.arange(1, ntr + 1) * nsamp, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=1000.0, trialdefinition=trl)
    out = "pow"
    got = spy.freqanalysis(data, method=method, output=out, precision="reference", **kw)
    ref = spy.freqanalysis(data, method=method, output=out, compute_method="sequential", routine_classes=ORACLE_FREQ, **kw)
    assert_parity(got.data, ref.data, what=method)
    err = np.abs(got.data.astype(np.float64) - ref.data)
    assert (err <= 1e-5 * np.abs(ref.data)).mean() >= 0.99


def test_reference_precision_of_wavelets_and_superlets():
    """precision="reference" for the wavelet methods (cwt64_kernel.h: float64 FFT convolutions, complex64 rounding where
    cwt_time / cwtSL store their result).  The reference's own scipy.signal.fftconvolve transforms the float32 trial in
    SINGLE precision (error 1.5e-7 of the largest coefficient), so the yardstick is the oracle fed float64 trials: with a
    5 Hz line 60 dB above the noise the high-frequency scales - made of the noise alone - are exact to float32 rounding
    under precision="reference" and carry the line's transform error in the default kernels (and in the reference)."""
    import syncopy_amd as spy
    from oracle_routines import ORACLE_FREQ, float64_fftconvolve
    from parity import excess
    rng = np.random.default_rng(21)
    nsamp, ntr, nchan = 3000, 2, 3
    t = np.arange(nsamp * ntr) / 1000.0
    x = rng.normal(size=(nsamp * ntr, nchan)) + 1000.0 * np.sin(2 * np.pi * 5.0 * t)[:, None]
    trl = np.stack([np.arange(ntr) * nsamp, np.arange(1, ntr + 1) * nsamp, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=1000.0, trialdefinition=trl)
    for kw in (dict(method="wavelet", foi=np.array([40.0, 90.0, 200.0]), output="fourier"),
               dict(method="wavelet", foi=np.array([60.0, 150.0]), output="pow", toi=np.arange(0.5, 2.5, 0.01)),
               dict(method="superlet", foi=np.array([50.0, 120.0, 250.0]), order_max=4, c_1=2, adaptive=True, output="abs")):
        ref = spy.freqanalysis(data, compute_method="sequential", routine_classes=ORACLE_FREQ, polyremoval=0, **kw)
        with float64_fftconvolve():
            ref64 = spy.freqanalysis(data, compute_method="sequential", routine_classes=ORACLE_FREQ, polyremoval=0, **kw)
        exact = spy.freqanalysis(data, precision="reference", polyremoval=0, **kw)
        fast = spy.freqanalysis(data, polyremoval=0, **kw)
        b = np.asarray(ref64.data)

        def pure(a):
            err = np.abs(np.asarray(a).astype(np.complex128 if np.iscomplexobj(b) else np.float64) - b)
            return float((err <= 2e-5 * np.abs(b)).mean())
        fr64, fr32, frref = pure(exact.data), pure(fast.data), pure(ref.data)
        print(f"{kw['method']} {kw['output']}: elements within pure rtol 2e-5 of the float64 oracle - precision='reference' "
              f"{100 * fr64:.2f} %, default kernels {100 * fr32:.1f} %, the reference's own single-precision transform {100 * frref:.1f} %")
        assert fr64 >= 0.99 and fr64 > fr32, (kw["method"], fr64, fr32)
        # (against the REFERENCE this data set shows the reference's own single-precision transform error - up to 5e-6 of
        # a coefficient here; the float64 result is held to the float64 oracle by the criterion as well)
        assert excess(exact.data, ref64.data) <= 1.0
