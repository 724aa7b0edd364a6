"""The host table builders of the tapered FFT (syncopy_amd/csrc/host_fft.h) against NumPy.  The library uploads what they
return and the kernel emulator points its arguments at the same vectors (mtmfft_tables.h); here they are compiled with the
host compiler alone (no HIP, no device) and asked through a small C shim."""
import ctypes as C

import numpy as np
import pytest

import build_emu



@pytest.fixture(scope="module")
def lib():
    return build_emu.build_shim("tables_shim.cpp", "libspytables.so")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_taper_moments_and_prescaled_windows(lib):
    rng = np.random.default_rng(0)
    for K, nsig in [(1, 1), (3, 7), (2, 1000), (7, 4097)]:
        tap = rng.normal(size=(K, nsig))
        tf = np.ascontiguousarray(tap, dtype=np.float32)
        got = np.zeros((K, 2))
        lib.shim_taper_moments(_ptr(tf), K, nsig, _ptr(got))
        w = tf.astype(np.float64)
        lever = np.arange(nsig) - 0.5 * (nsig - 1)
        # float64 sums of exactly representable terms in two orders (sequential there, pairwise here): n eps of sum |term|
        for col, terms in ((0, w), (1, w * lever)):
            bound = nsig * np.finfo(np.float64).eps * np.abs(terms).sum(axis=1)
            assert (np.abs(got[:, col] - terms.sum(axis=1)) <= bound).all(), (K, nsig, col)
        scale = 0.37
        half = np.zeros((K, nsig), np.float32)
        lib.shim_taper_half(_ptr(tap), C.c_longlong(tap.size), C.c_double(scale), _ptr(half))
        np.testing.assert_array_equal(half, (tap * (0.5 * scale)).astype(np.float32))       # the same two float64 products


def _fpos(lib, freq_idx, nf):
    fi = np.ascontiguousarray(freq_idx, dtype=np.int32)
    fpos, ident, msg = np.full(nf, -7, np.int32), C.c_int(-1), C.create_string_buffer(128)
    rc = lib.shim_fpos_map(_ptr(fi), len(fi), nf, _ptr(fpos), C.byref(ident), msg, 128)
    return rc, fpos, ident.value, msg.value.decode()


def test_frequency_map(lib):
    rc, fpos, ident, msg = _fpos(lib, [5, 0, 8, 3], 9)
    assert (rc, ident, msg) == (0, 0, "")
    np.testing.assert_array_equal(fpos, [1, -1, -1, 3, -1, 0, -1, -1, 2])
    rc, fpos, ident, _ = _fpos(lib, np.arange(9), 9)
    assert (rc, ident) == (0, 1)
    np.testing.assert_array_equal(fpos, np.arange(9))
    assert _fpos(lib, np.arange(8), 9)[2] == 0                   # in order but not every bin
    assert _fpos(lib, [1, 0, 2], 3)[2] == 0                      # every bin but not in order
    # the two refusals, with the messages spyhip_fft_plan_create reports
    rc, _, _, msg = _fpos(lib, [0, 9], 9)
    assert rc == -1 and msg == "freq_idx[1]=9 outside [0,9)"
    rc, _, _, msg = _fpos(lib, [2, -1], 9)
    assert rc == -1 and msg == "freq_idx[1]=-1 outside [0,9)"
    rc, _, _, msg = _fpos(lib, [4, 2, 4], 9)
    assert rc == -1 and msg == "freq_idx holds duplicate bin 4"


def test_twiddles(lib):
    for n, count in [(16, 16), (2000, 501), (12000, 3001)]:
        got = np.zeros((count, 2), np.float32)
        lib.shim_twiddles(n, count, _ptr(got))
        ang = -2.0 * np.pi * np.arange(count) / n
        np.testing.assert_array_equal(got, np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32))


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("nfft,M,M1", [(7, 16, 0), (500, 1024, 0), (900, 4096, 64)])
def test_bluestein_tables(lib, nfft, M, M1, wide):
    """chirp[n] = exp(-i pi n^2 / nfft) element by element, and bhat = FFT_M of the wrapped conjugate chirp / M: transformed
    back in float64 it reproduces that sequence.  Observed max |M ifft(bhat) - b| with float32 storage: 4.0e-8, 7.2e-8, 4.3e-8
    for the three shapes (float64 storage: 3.4e-16, 1.4e-15, 1.1e-15)."""
    dt = np.float64 if wide else np.float32
    chirp, bhat = np.zeros((nfft, 2), dt), np.zeros((M, 2), dt)
    lib.shim_bluestein(nfft, M, M1, wide, _ptr(chirp), _ptr(bhat))
    n = np.arange(nfft, dtype=np.int64)
    ang = np.pi * ((n * n) % (2 * nfft)) / nfft                   # the closed form, phase reduced exactly
    want = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    # unit-modulus values: one rounding to the storage type, half an ulp of 1 at the most (float64: plus libm's last bit)
    assert np.abs(chirp - want).max() <= (2.0 ** -52 if wide else 2.0 ** -24)
    b = np.zeros(M, np.complex128)
    b[:nfft] = np.exp(1j * ang)
    b[M - n[1:]] = b[n[1:]]
    B = bhat[:, 0].astype(np.float64) + 1j * bhat[:, 1]
    if M1:                                                         # stored [k1][k2] with k = k1 + M1 k2
        B = B.reshape(M1, M // M1).T.reshape(-1)
    err = np.abs(np.fft.ifft(B) * M - b).max()                     # relative to |b| = 1
    print(f"bluestein_tables({nfft}, {M}, {M1}, wide={wide}): max |M ifft(bhat) - b| = {err:.3g}")
    # float32 storage of the spectrum: one rounding, 6e-8, times a few.  float64: the radix-2 host transform, log2(M) eps times a few
    assert err <= (1e-12 if wide else 1e-6)
