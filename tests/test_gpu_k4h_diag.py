"""K4h's diagonal sub-tiles (csrc/csdh_kernel.h): in the 16 sub-tiles whose row block is their column block the kernel
accumulates S = Rh'Rh + Ih'Ih, P = Rh'Rl + Ih'Il and M = Ih'Rh + Ih'Rl + Il'Rh (7 matrix instructions per 32 rows
instead of 12) and forms Re = S + P + P', Im = M - M' once, in the epilogue.  Checked here at 256 channels x 3
frequencies and 1 ... 97 rows (a partial chunk, exactly one chunk, odd and even chunk counts: both plane-swap parities
and the parity fix-up of the epilogue):

  * the whole lower triangle (all 136 sub-tiles) against complex128 products of the same spectra, shared criterion;
  * inside every diagonal 16 x 16 block: Im of the diagonal exactly 0, Re bitwise symmetric, Im bitwise antisymmetric;
  * two strongly coherent channels 0.1 rad apart in the SAME block: the imaginary part of that entry within the
    criterion relative to itself (|d| <= (rtol + atol_rel) |b|: M - M' must not lose it to cancellation);
  * the validity rule: a zero channel (no flag, zeros), a NaN (flagged, float32 kernel, NaN propagates), a channel
    2^20 below its batch peak at one frequency (flagged, the float32 kernel's result);
  * a second launch into the same accumulator (33 rows, then 32): the launch adds."""
import functools

import numpy as np
import pytest

from parity import ATOL_REL, RTOL, assert_parity, excess

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C, F = 256, 3
ROWS = (1, 31, 32, 33, 64, 65, 97)
PAIR = (3, 11)          # the coherent pair of every 16-channel block: channels 16 b + 3 and 16 b + 11
LAG = 0.1               # rad


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


@functools.lru_cache(maxsize=None)
def _spectra(R, seed=0):
    """(R, F, C) complex64 noise with channel gains 18 decades apart; in every block channel 16 b + 11 is channel
    16 b + 3 turned by LAG plus 1 % of noise of its own (coherence ~0.9999).  Built once per shape; nobody writes to it."""
    g = torch.Generator(device="cuda").manual_seed(7000 + 10 * R + seed)
    x = torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, device="cuda", dtype=torch.float32))
    turn = complex(np.cos(LAG), np.sin(LAG))
    for b in range(16):
        x[:, :, 16 * b + PAIR[1]] = x[:, :, 16 * b + PAIR[0]] * turn + 0.01 * x[:, :, 16 * b + PAIR[1]]
    perm = torch.randperm(C, generator=torch.Generator(device="cuda").manual_seed(1234), device="cuda")     # the same gains in every set
    x = x * torch.logspace(-14, 4, C, device="cuda", dtype=torch.float32)[perm]
    return x.contiguous()


def _reference(spec, f):
    x = spec[:, f, :].to(torch.complex128)
    return (x.T @ x.conj()).cpu().numpy()


def _norm(ref):
    d = np.sqrt(np.real(np.diag(ref)))
    d[d == 0] = 1.0
    return np.outer(d, d)


def _check_parity(spec, acc, freqs, what):
    """All 136 sub-tiles: the lower triangle, coherency-normalised (the channel scales differ by 18 decades)."""
    il = np.tril_indices(C)
    worst = 0.0
    for f in freqs:
        ref = _reference(spec, f)
        n = _norm(ref)
        got = acc[f].cpu().numpy()
        e = excess((got / n)[il].astype(np.complex64), (ref / n)[il].astype(np.complex64))
        worst = max(worst, e)
        assert e <= 1.0, f"{what} f={f}: parity violated, max err/tol = {e:.3g}"
    return worst


def _check_structure(acc, freqs, what):
    """What holds by construction inside the 16 diagonal blocks."""
    for f in freqs:
        got = acc[f].cpu().numpy()
        for b in range(16):
            blk = got[16 * b:16 * b + 16, 16 * b:16 * b + 16]
            re, im = np.ascontiguousarray(blk.real), np.ascontiguousarray(blk.imag)
            assert np.all(np.diag(im) == 0.0), f"{what} f={f} block {b}: Im of the diagonal"
            assert np.array_equal(re.view(np.uint32), re.T.copy().view(np.uint32)), f"{what} f={f} block {b}: Re not symmetric"
            # -x flips the sign bit and nothing else; +0 / -0 compare equal as numbers and are both admitted
            assert np.array_equal(im, -im.T) and np.array_equal(np.abs(im).view(np.uint32), np.abs(im.T).copy().view(np.uint32)), \
                f"{what} f={f} block {b}: Im not antisymmetric"


def _check_pairs(spec, acc, freqs, what):
    """Im of the coherent pair of every block against complex128, relative to itself."""
    worst = 0.0
    for f in freqs:
        ref = _reference(spec, f)
        got = acc[f].cpu().numpy()
        for b in range(16):
            i, j = 16 * b + PAIR[1], 16 * b + PAIR[0]
            r, a = ref[i, j].imag, float(got[i, j].imag)
            assert abs(r) > 0.02 * np.sqrt(ref[i, i].real * ref[j, j].real), "the pair is coherent with a lag"
            e = abs(a - r) / ((RTOL + ATOL_REL) * abs(r))
            worst = max(worst, e)
            assert e <= 1.0, f"{what} f={f} block {b}: Im of the coherent pair, err/tol = {e:.3g}"
    return worst


@pytest.mark.parametrize("R", ROWS)
def test_lower_triangle_structure_and_coherent_pairs(be, R):
    spec = _spectra(R)
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    assert be.csd_split_fallbacks() == 0
    e = _check_parity(spec, acc, range(F), f"R={R}")
    _check_structure(acc, range(F), f"R={R}")
    p = _check_pairs(spec, acc, range(F), f"R={R}")
    print(f"[k4h diag] R={R}: lower triangle err/tol = {e:.3g}, Im of same-block coherent pairs err/tol = {p:.3g}")
    again = torch.zeros_like(acc)
    be.csd_accumulate(spec, again)
    assert torch.equal(torch.view_as_real(acc), torch.view_as_real(again)), "deterministic"


@pytest.mark.parametrize("R", ROWS)
def test_validity_zero_channel(be, R):
    """A channel of zeros: nothing to flag, its rows and columns stay zero, the rest is unchanged."""
    spec = _spectra(R).clone()
    spec[:, :, 37] = 0
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    assert be.csd_split_fallbacks() == 0
    assert float(acc[:, 37, :].abs().max()) == 0.0 and float(acc[:, :, 37].abs().max()) == 0.0
    _check_parity(spec, acc, range(F), f"zero channel, R={R}")
    _check_structure(acc, range(F), f"zero channel, R={R}")


@pytest.mark.parametrize("R", ROWS)
def test_validity_nan_row(be, R):
    """A NaN at one frequency: that frequency is flagged and redone by the float32 kernel, where the NaN reaches the
    rows / columns of its channel; the other frequencies are added by K4h as if nothing had happened."""
    spec = _spectra(R).clone()
    spec[R // 2, 1, 40] = float("nan")
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    assert be.csd_split_fallbacks() == 1
    assert bool(torch.isnan(acc[1, 40, :41].real).all()) and bool(torch.isnan(acc[1, 200, 40].real))
    assert bool(torch.isfinite(torch.view_as_real(acc[0])).all()) and bool(torch.isfinite(torch.view_as_real(acc[2])).all())
    _check_parity(spec, acc, (0, 2), f"NaN at f=1, R={R}")
    _check_structure(acc, (0, 2), f"NaN at f=1, R={R}")


@pytest.mark.parametrize("R", ROWS)
def test_validity_channel_below_its_peak(be, R):
    """One channel 2^20 below its batch peak at one frequency: the fp16 pair cannot hold it, the frequency is flagged and
    the float32 kernel adds it - the very numbers `split=False` gives there - while the other frequencies stay on K4h."""
    spec = _spectra(R).clone()
    spec[:, 2, 90] *= 2.0 ** -20
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    assert be.csd_split_fallbacks() == 1
    _check_parity(spec, acc, range(F), f"2^-20 at f=2, R={R}")
    _check_structure(acc, (0, 1), f"2^-20 at f=2, R={R}")
    f32 = torch.zeros_like(acc)
    be.csd_accumulate(spec, f32, split=False)
    il = torch.tril_indices(C, C, device="cuda")
    assert torch.equal(torch.view_as_real(acc[2][il[0], il[1]]), torch.view_as_real(f32[2][il[0], il[1]])), "the float32 kernel's result"


def test_second_launch_adds(be):
    """33 rows, then 32 into the same accumulator (odd, then even parity of the chunk count): acc +=, not acc =."""
    a, b = _spectra(33), _spectra(32, seed=1)
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(a, acc)
    first = acc.clone()
    be.csd_accumulate(b, acc)
    assert be.csd_split_fallbacks() == 0
    assert not torch.equal(torch.view_as_real(acc), torch.view_as_real(first))
    both = torch.cat((a, b)).contiguous()
    _check_parity(both, acc, range(F), "33 + 32 rows")
    _check_structure(acc, range(F), "33 + 32 rows")
    _check_pairs(both, acc, range(F), "33 + 32 rows")
