"""K4h's wave roles (csrc/csdh_kernel.h): of the two waves that share a SIMD one only multiplies (off-diagonal sub-tiles)
and the other fetches, splits and writes the whole chunk's rows 8 L ... 8 L + 7 in four phases (row half x channel half,
16-byte loads) next to its own, smaller share of sub-tiles, the 16 diagonal ones among them.  Which wave owns a sub-tile
does not change its arithmetic, so everything below is the criterion the kernel met before; what can go wrong is the
loader (a phase writing the wrong rows or channels, the tail of the last chunk) and the table (a sub-tile dealt twice or
not at all).  256 channels, F in {1, 3}, rows 1 ... 97: partial and full 8-row loader groups (1, 7, 8, 9), partial and
full 4-row phases, partial and full chunks (25, 31, 32, 33), both parities of the chunk count (64, 65, 97):

  * the whole lower triangle against complex128 products of the same spectra, coherency-normalised (channel gains 18
    decades apart: a value that lands in the wrong channel or row group is wrong by decades in that channel's own
    rows and columns), shared criterion;
  * a second launch into the same accumulator;
  * a frequency range that does not start at 0 (spyhip_csd_accumulate_split_range, the route of coh_pipeline): the
    range is added, the frequencies outside it are left alone."""
import functools

import numpy as np
import pytest

from parity import excess

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C = 256
ROWS = (1, 7, 8, 9, 25, 31, 32, 33, 64, 65, 97)


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


@functools.lru_cache(maxsize=None)
def _spectra(R, F, seed=0):
    """(R, F, C) complex64 noise, every third channel coupled to a common source, channel gains 18 decades apart in a
    fixed random order.  Built once per shape; nobody writes to it."""
    g = torch.Generator(device="cuda").manual_seed(9000 + 100 * R + 10 * F + seed)
    x = torch.view_as_complex(torch.randn((R, F, C, 2), generator=g, device="cuda", dtype=torch.float32))
    src = torch.view_as_complex(torch.randn((R, F, 1, 2), generator=g, device="cuda", dtype=torch.float32))
    x[:, :, ::3] += 0.8 * src
    perm = torch.randperm(C, generator=torch.Generator(device="cuda").manual_seed(4321), device="cuda")
    x = x * torch.logspace(-14, 4, C, device="cuda", dtype=torch.float32)[perm]
    return x.contiguous()


def _reference(spec, f):
    x = spec[:, f, :].to(torch.complex128)
    return (x.T @ x.conj()).cpu().numpy()


def _check_parity(spec, acc, freqs, what):
    """All 136 sub-tiles: the lower triangle, coherency-normalised."""
    il = np.tril_indices(C)
    worst = 0.0
    for f in freqs:
        ref = _reference(spec, f)
        d = np.sqrt(np.real(np.diag(ref)))
        d[d == 0] = 1.0
        n = np.outer(d, d)
        got = acc[f].cpu().numpy()
        e = excess((got / n)[il].astype(np.complex64), (ref / n)[il].astype(np.complex64))
        worst = max(worst, e)
        assert e <= 1.0, f"{what} f={f}: parity violated, max err/tol = {e:.3g}"
    return worst


@pytest.mark.parametrize("F", (1, 3))
@pytest.mark.parametrize("R", ROWS)
def test_lower_triangle(be, R, F):
    spec = _spectra(R, F)
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc)
    assert be.csd_split_fallbacks() == 0
    e = _check_parity(spec, acc, range(F), f"R={R} F={F}")
    print(f"[k4h roles] R={R} F={F}: lower triangle err/tol = {e:.3g}")


@pytest.mark.parametrize("F", (1, 3))
def test_second_launch_adds(be, F):
    """97 rows, then 25 into the same accumulator: acc +=, not acc =."""
    a, b = _spectra(97, F), _spectra(25, F, seed=1)
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(a, acc)
    first = acc.clone()
    be.csd_accumulate(b, acc)
    assert be.csd_split_fallbacks() == 0
    assert not torch.equal(torch.view_as_real(acc), torch.view_as_real(first))
    _check_parity(torch.cat((a, b)).contiguous(), acc, range(F), f"97 + 25 rows, F={F}")


@pytest.mark.parametrize("R", (9, 33, 97))
def test_frequency_range_not_from_zero(be, R):
    """f0 = 1, nf = 1 of F = 3: frequency 1 is added, frequencies 0 and 2 keep what they held."""
    F = 3
    spec = _spectra(R, F)
    absmax = torch.view_as_real(spec).abs().amax(dim=(0, 1, 3)).contiguous()
    marker = complex(3.0, -5.0)
    acc = torch.full((F, C, C), marker, dtype=torch.complex64, device="cuda")
    ctx = be.context(spec.device)
    ctx.bind_stream()
    be.check(ctx.lib.spyhip_csd_accumulate_split_range(ctx.handle, be._ptr(spec), R, F, C, be._ptr(acc), be._ptr(absmax), 1, 1),
             "spyhip_csd_accumulate_split_range")
    torch.cuda.synchronize()
    assert be.csd_split_fallbacks() == 0
    for f in (0, 2):
        assert bool((acc[f] == marker).all()), f"frequency {f} lies outside the range"
    il = torch.tril_indices(C, C, device="cuda")
    added = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    added[1][il[0], il[1]] = acc[1][il[0], il[1]] - marker
    # next to (3, -5) an entry of a channel pair with small gains is rounded away, so the parity check runs on a launch
    # of the same range into zeros, and the launch into the marker must be that result after the same two roundings
    clean = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.check(ctx.lib.spyhip_csd_accumulate_split_range(ctx.handle, be._ptr(spec), R, F, C, be._ptr(clean), be._ptr(absmax), 1, 1),
             "spyhip_csd_accumulate_split_range")
    torch.cuda.synchronize()
    assert float(clean[0].abs().max()) == 0.0 and float(clean[2].abs().max()) == 0.0
    _check_parity(spec, clean, (1,), f"range [1, 2) of 3, R={R}")
    want = (clean[1][il[0], il[1]] + marker) - marker           # the same two float32 roundings the accumulator saw
    assert torch.equal(torch.view_as_real(added[1][il[0], il[1]]), torch.view_as_real(want)), "acc[1] = marker + products"
