"""The wavelet plan at reference precision (cwt64_kernel.h, spyhip_cwt_plan_set_precision) against the float64 oracle,
held to float32 rounding element by element (cwt64_ref.py), and the slot bound of the direct kernels (cwt_direct_fits)."""
import numpy as np
import pytest

from oracle import spy_oracle as O
from parity import assert_parity
from cwt64_ref import assert_cwt64, cwt64_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OUTPUTS = ("pow", "abs", "real", "imag", "fourier")
FAMILIES = {"Morlet": {}, "MorletSL": {"sl_cycles": 3.0}, "Paul": {"family": "Paul", "order": 4},
            "DOG": {"family": "DOG", "order": 2}}


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


def _data(seed, rows, ncol, offset=0.5):
    rng = np.random.default_rng(seed)
    t = np.arange(rows)[:, None] / 1000.0
    return (rng.normal(size=(rows, ncol)) + offset + 3.0 * np.sin(2 * np.pi * 40.0 * t + np.arange(ncol))).astype("f4")


def _plan(be, nsig, nchan, scales, output, detrend=0, tpos=None, nto=None, reference=True, **fam):
    plan = be.CWTPlan(nsig, nchan, scales, 1e-3, detrend=detrend, output=output, tpos=tpos, ntime_out=nto, **fam)
    if reference:
        assert plan.set_precision(True)
    return plan


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _exec(plan, d, ss, lo, hi, chan_idx=None, out=None, accumulate=0):
    ci = None if chan_idx is None else torch.tensor(np.asarray(chan_idx, dtype=np.int32), device="cuda")
    sst, lot, hit = _dev(np.asarray(ss, dtype=np.int64), np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64))
    r = plan.execute(d, sst, lot, hit, chan_idx=ci, out=out, accumulate=accumulate)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("nchan", [1, 5, 64])
def test_plan_every_family_and_output(be, family, nchan):
    """Morlet, MorletSL, Paul and DOG taps, every output kind, one / an odd number of (selected, one repeated) / 64
    channels, the pre-selection inside the trial."""
    nsig = 357
    fam = FAMILIES[family]
    ncol = 7 if nchan == 5 else nchan
    data = _data(nchan, 2 * nsig + 80, ncol)
    ci = [6, 2, 6, 0, 3] if nchan == 5 else None
    ss, lo, hi = np.array([13, nsig + 50]), np.array([0, nsig + 40]), np.array([nsig + 30, 2 * nsig + 80])
    scales = np.array([0.004, 0.0015]) if "sl_cycles" in fam else np.array([0.03, 0.008, 0.002])
    (d,) = _dev(data)
    amax = float(np.abs(cwt64_ref(data, ss, lo, hi, nsig, scales, 0, "fourier", chan_idx=ci, **fam)).max())
    for output in OUTPUTS:
        plan = _plan(be, nsig, nchan, scales, output, **fam)
        got = _exec(plan, d, ss, lo, hi, chan_idx=ci).cpu().numpy()
        ref = cwt64_ref(data, ss, lo, hi, nsig, scales, 0, output, chan_idx=ci, **fam)
        assert_cwt64(got, ref, output, f"{family} {nchan} ch {output}", amax=amax)


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_plan_accumulation_and_selection(be, output):
    """accumulate 1 (out[b] += segment b), accumulate 2 summed over two calls, a post-selection (tpos) whose unused slots
    stay untouched; detrend -1 and 1 (the latter held to parity: float64 line fit against the reference's float32 lstsq)."""
    nsig, nchan = 400, 3
    data = _data(9, 4 * nsig + 40, nchan)
    ss = np.arange(4) * (nsig + 10) + 5
    lo, hi = ss - 5, ss + nsig + 5
    scales = np.array([0.02, 0.005])
    (d,) = _dev(data)
    ref = cwt64_ref(data, ss, lo, hi, nsig, scales, -1, output)
    plan = _plan(be, nsig, nchan, scales, output, detrend=None)
    got = _exec(plan, d, ss, lo, hi).cpu().numpy()
    assert_cwt64(got, ref, output, f"detrend -1 {output}")
    rng = np.random.default_rng(2)
    base = torch.from_numpy(rng.normal(size=got.shape).astype(got.dtype)).cuda()
    acc = _exec(plan, d, ss, lo, hi, out=base.clone(), accumulate=1).cpu().numpy()
    b = base.cpu().numpy().astype(np.complex128)
    r = ref.astype(np.complex128)
    assert_cwt64(acc - b, r, output, f"accumulate 1 {output}", scale=np.abs(r) + np.abs(b + r))
    tot = torch.zeros(plan.out_shape(1), dtype=plan.out_dtype, device="cuda")
    _exec(plan, d, ss[:3], lo[:3], hi[:3], out=tot, accumulate=2)
    _exec(plan, d, ss[3:], lo[3:], hi[3:], out=tot, accumulate=2)
    assert_cwt64(tot.cpu().numpy(), r.sum(axis=0, keepdims=True), output, f"accumulate 2 {output}", nterms=4,
                 scale=np.abs(r).sum(axis=0, keepdims=True))
    keep = np.r_[0:4, 50:390:11, 399]
    tpos = np.full(nsig, -1, dtype=np.int32)
    tpos[keep] = 3 * np.arange(keep.size) + 2
    nto = 3 * keep.size + 2
    sel_plan = _plan(be, nsig, nchan, scales, output, detrend=0, tpos=tpos, nto=nto)
    fill = torch.full(sel_plan.out_shape(4), 0.5, dtype=sel_plan.out_dtype, device="cuda")
    sel = _exec(sel_plan, d, ss, lo, hi, out=fill.clone(), accumulate=1).cpu().numpy()
    ref0 = cwt64_ref(data, ss, lo, hi, nsig, scales, 0, output)
    gap = np.ones(nto, dtype=bool)
    gap[tpos[keep]] = False
    assert np.all(sel[:, gap] == 0.5)
    assert_cwt64(sel[:, tpos[keep]] - 0.5, ref0[:, keep], output, f"tpos {output}",
                 scale=np.abs(ref0[:, keep]).astype(np.float64) + np.abs(ref0[:, keep] + 0.5))
    lin = _plan(be, nsig, nchan, scales, output, detrend=1)
    assert_parity(_exec(lin, d, ss, lo, hi).cpu().numpy(), cwt64_ref(data, ss, lo, hi, nsig, scales, 1, output),
                  what=f"detrend 1 {output}")


def _check_corners(got_dev, data, ss, lo, hi, nsig, scales, output, nchan, summed=False):
    """The first and last segment and channel of a large run against the oracle."""
    segs, chans = [0, len(ss) - 1], [0, nchan - 1]
    if summed:
        got = got_dev[:, :, :, chans].cpu().numpy()
        r = cwt64_ref(data[:, :nchan], ss, lo, hi, nsig, scales, 0, output, chan_idx=chans).astype(np.complex128)
        assert_cwt64(got, r.sum(axis=0, keepdims=True), output, f"{len(ss)}-segment sum {output}", nterms=len(ss),
                     scale=np.abs(r).sum(axis=0, keepdims=True))
        return
    got = got_dev[segs][:, :, :, chans].cpu().numpy()
    ref = cwt64_ref(data[:, :nchan], ss[segs], lo[segs], hi[segs], nsig, scales, 0, output, chan_idx=chans)
    assert_cwt64(got, ref, output, f"corners {output}")


def test_second_kernel_launch(be):
    """128 channels x 90 segments of 2000 samples (L = 4096): 11 520 (segment, channel) items, more than the ~10 900 that
    one launch's work arrays hold (2 GiB / (3 L x 16 B)) - the second launch starts at wg0 > 0."""
    nsig, nchan, nseg = 2000, 128, 90
    rng = np.random.default_rng(5)
    data = (rng.normal(size=(nseg * nsig, nchan)) + 0.25).astype("f4")
    ss = np.arange(nseg) * nsig
    lo, hi = ss, ss + nsig
    scales = np.array([0.01, 0.003])
    (d,) = _dev(data)
    plan = _plan(be, nsig, nchan, scales, "fourier")
    assert nseg * nchan > (2 << 30) // (3 * 4096 * 16)
    _check_corners(_exec(plan, d, ss, lo, hi), data, ss, lo, hi, nsig, scales, "fourier", nchan)


def test_second_segment_chunk(be):
    """20 scales x 128 channels x 4000 samples complex: 82 MB of staging per segment, 60 segments more than the 4 GiB one
    chunk holds - the second chunk (seg0 > 0) per segment and summed (accumulate 2 adds to what the first chunk left)."""
    nsig, nchan, nseg, nsc = 4000, 128, 60, 20
    assert nsc * nchan * nsig * 8 * nseg > (4 << 30)
    rng = np.random.default_rng(6)
    data = (rng.normal(size=(nseg * nsig, nchan)) - 0.4).astype("f4")
    ss = np.arange(nseg) * nsig
    lo, hi = ss, ss + nsig
    scales = np.geomspace(0.02, 0.0015, nsc)
    (d,) = _dev(data)
    plan = _plan(be, nsig, nchan, scales, "fourier")
    out = _exec(plan, d, ss, lo, hi)
    _check_corners(out, data, ss, lo, hi, nsig, scales, "fourier", nchan)
    del out
    torch.cuda.empty_cache()
    tot = torch.zeros(plan.out_shape(1), dtype=plan.out_dtype, device="cuda")
    _exec(plan, d, ss, lo, hi, out=tot, accumulate=2)
    _check_corners(tot, data, ss, lo, hi, nsig, scales, "fourier", nchan, summed=True)


def test_the_bound_separates_the_precisions(be):
    """A 5 Hz line 60 dB above the noise: the high-frequency scales are made of the noise alone.  The float64 plan holds
    every element to float32 rounding; the float32 kernels (absolute error ~5e-7 of the largest coefficient) miss that
    bound on a clear share of them."""
    nsig, nchan = 3000, 3
    rng = np.random.default_rng(21)
    t = np.arange(nsig) / 1000.0
    data = (rng.normal(size=(nsig, nchan)) + 1000.0 * np.sin(2 * np.pi * 5.0 * t)[:, None]).astype("f4")
    ss, lo, hi = np.array([0]), np.array([0]), np.array([nsig])
    scales = np.array([0.03, 0.004, 0.0025, 0.0015])
    ref = cwt64_ref(data, ss, lo, hi, nsig, scales, 0, "fourier").astype(np.complex128)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-12 * np.abs(ref).max()
    (d,) = _dev(data)
    miss = {}
    for reference in (True, False):
        plan = _plan(be, nsig, nchan, scales, "fourier", reference=reference)
        got = _exec(plan, d, ss, lo, hi).cpu().numpy().astype(np.complex128)
        miss[reference] = float((np.abs(got - ref) > bound).mean())
    print(f"share of elements beyond float32 rounding: reference {miss[True]:.4f}, float32 kernels {miss[False]:.3f}")
    assert miss[True] == 0.0
    assert miss[False] > 0.25, miss


def test_set_precision_length_limit(be):
    """The float64 path takes convolutions up to 2^22 points: nsig + taps - 1 = 2^22 is accepted, one more refused (plans
    only, nothing executed)."""
    taps = O.cwt_kernel(0.002, 1e-3).size
    assert taps < 100
    nsig = (1 << 22) - taps + 1
    assert be.CWTPlan(nsig, 1, [0.002], 1e-3, output="pow").set_precision(True)
    assert not be.CWTPlan(nsig + 1, 1, [0.002], 1e-3, output="pow").set_precision(True)


# ---- front end: precision="reference" against the oracle fed float64 trials ------------------------------------------
def _front(kw, polyremoval, select=None, sharp=True):
    import syncopy_amd as spy
    from oracle_routines import ORACLE_FREQ, float64_fftconvolve
    rng = np.random.default_rng(31)
    nsamp, ntr, nchan = 1500, 3, 4
    t = np.arange(nsamp * ntr) / 1000.0
    x = rng.normal(size=(nsamp * ntr, nchan)) + 50.0 * np.sin(2 * np.pi * 12.0 * t)[:, None] + 3.0
    trl = np.stack([np.arange(ntr) * nsamp, np.arange(1, ntr + 1) * nsamp, np.zeros(ntr)], axis=1)
    data = spy.AnalogData(x.astype(np.float32), samplerate=1000.0, trialdefinition=trl)
    if select is not None:
        kw = dict(kw, select=select)
    with float64_fftconvolve():
        ref = spy.freqanalysis(data, compute_method="sequential", routine_classes=ORACLE_FREQ, polyremoval=polyremoval, **kw)
    got = spy.freqanalysis(data, precision="reference", polyremoval=polyremoval, **kw)
    g, r = np.asarray(got.data), np.asarray(ref.data)
    assert g.shape == r.shape
    assert_parity(g, r, what=str(kw))
    if sharp:
        err = np.abs(g.astype(np.complex128) - r)
        frac = float((err <= 2e-5 * np.abs(r)).mean())
        assert frac >= 0.99, (kw, frac)


@pytest.mark.parametrize("case", ["trial_average", "linear_detrend", "channel_select", "toi_off_grid"])
def test_front_end_wavelet_reference(be, case):
    kw = dict(method="wavelet", foi=np.array([8.0, 30.0, 120.0]), output="pow")
    if case == "trial_average":
        _front(dict(kw, keeptrials=False), 0)
    elif case == "linear_detrend":
        _front(dict(kw, output="fourier"), 1, sharp=False)
    elif case == "channel_select":
        _front(dict(kw, output="abs"), 0, select={"channel": [0, 2]})
    else:
        # (the reference takes equidistant toi arrays only: a stride of 37.1 samples from off the sample grid)
        _front(dict(kw, toi=np.arange(0.1033, 1.4, 0.0371)), 0)


@pytest.mark.parametrize("adaptive", [False, True])
def test_front_end_superlet_reference(be, adaptive):
    _front(dict(method="superlet", foi=np.array([20.0, 60.0, 150.0]), order_max=4, c_1=2, adaptive=adaptive,
                output="pow"), 0)


# ---- the direct kernels' slot bound (cwt_direct_fits): plans only, then gapped slots below the bound executed -----------
def test_direct_kernels_refuse_gapped_plans_beyond_the_bound(be):
    """tpos[n] = 10000 n: a 1024-point block's ~990 samples span ~9.9e6 slots.  At 32 complex channels x 2 scales (512
    bytes per slot) that is beyond 32-bit store offsets: the plan is staged only and set_direct(True) fails; at 16
    channels it is within them.  A contiguous production-shaped plan (c4: 128 channels, 25 scales 4 ... 100 Hz) keeps the
    direct kernels.  Nothing is executed."""
    from syncopy_amd._lib import SpyHipError
    nsig = 2048
    tpos = (10000 * np.arange(nsig)).astype(np.int32)
    nto = int(tpos[-1]) + 1
    scales = [0.002, 0.003]
    far = be.CWTPlan(nsig, 32, scales, 1e-3, detrend=0, output="fourier", tpos=tpos, ntime_out=nto)
    with pytest.raises(SpyHipError):
        far.set_direct(True)
    far.set_direct(False)
    near = be.CWTPlan(nsig, 16, scales, 1e-3, detrend=0, output="fourier", tpos=tpos, ntime_out=nto)
    near.set_direct(True)
    w0 = 6.0
    c4 = (w0 + np.sqrt(2 + w0 ** 2)) / (4 * np.pi * np.arange(4.0, 104.0, 4.0))
    for output in ("pow", "fourier"):
        be.CWTPlan(16384, 128, c4, 1e-3, detrend=0, output=output).set_direct(True)


@pytest.mark.parametrize("output", ["pow", "fourier"])
def test_direct_kernels_gapped_slots(be, output):
    """Slots far apart (tpos[n] = 7 n + 3) through the direct kernels and through staging: every sample in its slot,
    the slots between zero after a store and untouched by accumulate 1."""
    nsig, nchan = 1400, 3
    rng = np.random.default_rng(4)
    data = rng.normal(size=(2 * nsig + 30, nchan)).astype("f4") + 1.5
    ss = np.array([10, nsig + 20])
    lo, hi = ss, ss + nsig
    scales = np.array([0.012, 0.004])
    tpos = (7 * np.arange(nsig) + 3).astype(np.int32)
    nto = 7 * nsig + 5
    gap = np.ones(nto, dtype=bool)
    gap[tpos] = False
    ref = np.stack([O.convert_output(O.cwt(O.detrend(np.array(data[a:a + nsig]), 0), 1000.0, scales).transpose(1, 0, 2), output)
                    for a in ss])
    (d,) = _dev(data)
    for direct in (True, False):
        plan = be.CWTPlan(nsig, nchan, scales, 1e-3, detrend=0, output=output, tpos=tpos, ntime_out=nto)
        plan.set_direct(direct)
        out = _exec(plan, d, ss, lo, hi).cpu().numpy()
        assert_parity(out[:, tpos], ref, what=f"gapped slots, direct={direct}")
        assert not out[:, gap].any()
        base = torch.full(plan.out_shape(2), 0.25, dtype=plan.out_dtype, device="cuda")
        acc = _exec(plan, d, ss, lo, hi, out=base, accumulate=1).cpu().numpy()
        assert np.all(acc[:, gap] == 0.25)
        assert_parity(acc[:, tpos] - np.float32(0.25), ref, what=f"gapped slots, accumulate 1, direct={direct}")
