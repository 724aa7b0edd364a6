"""The re-cut rule of the cross-spectral update (csd_route.h: recut_main) at its boundary on the device: the workgroups
beyond the last full round of the chip go to the re-cut tail when they fill at most a quarter of it."""
import numpy as np
import pytest

from parity import assert_parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C, R = 256, 70


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


@pytest.fixture(scope="module")
def spectra(be):
    """Spectra of the longer case; the shorter one reads its first frequencies."""
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(11)
    return n, torch.view_as_complex(torch.randn((R, n + n // 4 + 1, C, 2), generator=g, device="cuda", dtype=torch.float32))


@pytest.mark.parametrize("split", [False, True], ids=["float32", "half"])
@pytest.mark.parametrize("extra", [0, 1], ids=["quarter_round", "quarter_round_plus_1"])
def test_recut_boundary(be, spectra, extra, split):
    """256 channels, one workgroup per frequency on n compute units.  n + n/4 frequencies: the partial round fills exactly
    a quarter of the chip and is re-cut (rem * 4 == num_cu; its n/4 * 36 / 8 short workgroups already fill the chip, so
    its rows are not split).  One frequency more and the partial round stays in the main launch.  Both through the
    float32 entry and the half-precision one, against the complex128 product on the first and last frequency and on
    both sides of the cut, with the tolerances of test_csd_tail_row_split; a repeated call is bit-identical."""
    n, spec = spectra
    F = n + n // 4 + extra
    spec = spec[:, :F].contiguous()
    acc = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, acc, split=split)
    again = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.csd_accumulate(spec, again, split=split)
    assert torch.equal(torch.view_as_real(acc), torch.view_as_real(again))
    if split:
        assert be.csd_split_fallbacks() == 0
    be.csd_finalize(acc, 1.0 / R)
    for f in (0, n - 1, n, F - 1):
        x = spec[:, f, :].to(torch.complex128)
        ref = (x.T @ x.conj() / R).cpu().numpy()
        assert_parity(acc[f].cpu().numpy(), ref.astype(np.complex64), what=f"csd F={F} f={f}")


def test_kernel_name_through_the_library(be):
    """backend.csd_kernel_name asks the library (spyhip_csd_kernel_name), which asks the route with the context's
    arithmetic setting and the process's SPYHIP_CSD_F32."""
    import os
    half = "SPYHIP_CSD_F32" not in os.environ
    assert be.csd_kernel_name(256) == ("spycsd::csdh_kernel" if half else "spycsd::csd3m_kernel<256, 8, true, false, false>")
    assert be.csd_kernel_name(256, blocked=True) == "spycsd::csd3m_kernel<256, 8, true, false, false>"
    assert be.csd_kernel_name(300) == "spycsd::csd3m_kernel<304, 8, false>"
    assert be.csd_kernel_name(70, blocked=True) == "spycsd::csd_accum_kernel<3, 2, 0>"
    with be.csd_phase_exact(True):
        assert be.csd_kernel_name(300) == "spycsd::csd_accum_kernel<5, 4, 3>"
        assert be.csd_kernel_name(64) == "spycsd::csd_accum_kernel<5, 4, 2>"
    assert be.csd_kernel_name(300) == "spycsd::csd3m_kernel<304, 8, false>"
