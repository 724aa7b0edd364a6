"""Every transform length of the three schedule tables of syncopy_amd/csrc/mtmfft_route.h has an instance in the
translation units, under the name the route gives it, and that instance computes the transform: a table entry and a
`case` that part ways fail here.  The lengths are spelled out on purpose (tests/test_fft_route.py holds the route to its
tables); 200, 800, 1000, 2400, 2500 and 4000 run nowhere else on a device.

Every case runs complex spectra of every taper, 10000 also their taper mean (its pair form).  The power and taper-mean
epilogues of the other instances are not checked for correctness here: tests/test_gpu_kernels.py runs them for the lengths
it holds, and tools/fft_plan_dump.py only compares them between two builds."""
import numpy as np
import pytest

from parity import assert_parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEC = [100, 200, 300, 400, 500, 600, 768, 800, 1000, 1200, 1500, 1536, 1600, 2000, 2400, 2500, 3000, 3072, 3200, 4000,
       4800, 5000, 6000, 6144, 7500, 8000, 10000]
HALF = [12000, 12288, 15000, 16000, 16384, 20000]
DEC64 = [100, 200, 256, 300, 400, 500, 512, 600, 768, 800, 1000, 1024, 1200, 1500, 1536, 1600, 2000, 2048, 2400, 2500,
         3000, 3072, 3200, 4000, 4096, 4800, 5000, 6000, 6144, 7500, 8000, 8192, 10000]
NCHAN, GAP, SCALE = 5, 29, 0.5

# nfft, keeptapers, float32 name, float64 name (None: no float64 schedule)
CASES = [(n, True, ("HALF of " if n == 5000 else "") + f"N = {n},", f"mtmfft_dec64_kernel<N = {n}," if n in DEC64 else None)
         for n in DEC]
CASES += [(10000, False, "HALF of N = 10000,", "mtmfft_dec64_kernel<N = 10000,")]        # the taper mean takes the pair form
CASES += [(n, True, f"HALF of N = {n}" + ("," if n != 16384 else ">"), f"mtmfft_dec64_kernel<HALF of N = {n},") for n in HALF]
CASES += [(n, True, None, f"mtmfft_dec64_kernel<N = {n},") for n in DEC64 if n not in DEC]


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


@pytest.mark.parametrize("nfft,keep,name32,name64", CASES, ids=[f"N{c[0]}_{'keep' if c[1] else 'mean'}" for c in CASES])
def test_scheduled_length(be, nfft, keep, name32, name64):
    rng = np.random.default_rng(nfft)
    data = rng.normal(size=(2 * nfft + GAP + 4, NCHAN)).astype(np.float32)
    starts = [2, 2 + nfft + GAP]
    hann = np.hanning(nfft)
    tapers = np.stack([hann, hann * np.sin(2 * np.pi * 3 * np.arange(nfft) / nfft)])
    seg = np.stack([data[s:s + nfft] for s in starts]).astype(np.float64)                # (seg, n, chan)
    ref = SCALE * np.fft.rfft(tapers[None, :, :, None] * seg[:, None], axis=2)          # (seg, taper, freq, chan)
    if not keep:
        ref = ref.mean(axis=1, keepdims=True)
    plan = be.FFTPlan(nfft, nfft, NCHAN, tapers, SCALE, None, False, None, "fourier", keep)
    dev = torch.from_numpy(data).cuda()
    ss = torch.tensor(starts, dtype=torch.int64, device="cuda")
    if name32 is not None:
        assert name32 in plan.kernel_name and plan.kernel_name.startswith(("mtmfft_dec_kernel<", "mtmfft_quad_kernel<13, 1, ")), \
            plan.kernel_name
        assert_parity(plan.execute(dev, ss).cpu().numpy(), ref, what=plan.kernel_name)
    if name64 is not None:
        assert plan.set_precision(True)
        assert plan.kernel_name.startswith(name64), plan.kernel_name
        assert_parity(plan.execute(dev, ss).cpu().numpy(), ref, what=plan.kernel_name)
