"""The two pair kernels of the connectivity path on the device at their dispatch edges: K7 (ppc_accum_kernel with
ppc_accumulate_csd / ppc_finalize) and K9 (jack_coh_kernel).  K9 against the float64 model and rounding bound of
jack_oracle.py and against the replicate-by-replicate device loop it replaces; K7 against the oracle's walk over all
trial pairs; the launchers' refusals; one end-to-end jackknife with more than 16 tapers.  Every case prints its
err/tol (pytest -s)."""
import numpy as np
import pytest

import syncopy_amd as spy
import jack_oracle as JO
from oracle import spy_oracle as O
from oracle_routines import ORACLE_CONN
from parity import assert_parity, excess, jackknife_tolerances

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    from syncopy_amd import backend
    backend.require_gpu()
    return backend


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _sums(F, C, kind):
    return (torch.zeros((F, C, C), dtype=torch.complex128 if kind == "complex" else torch.float64, device="cuda"),
            torch.zeros((F, C, C), dtype=torch.float64, device="cuda"))


def _fused(be, spec, S, direct, kind, T, split):
    """K9 over the trials of spec (T, K, F, C) in launches of `split` trials."""
    _, K, F, C = spec.shape
    s, Sd, dd = _dev(spec), _dev(S), _dev(direct)
    sum_d, sum_d2 = _sums(F, C, kind)
    t0 = 0
    for n in split:
        be.jack_coh_accumulate(s[t0:t0 + n].reshape(-1, F, C).contiguous(), K, Sd, dd, kind, T, sum_d, sum_d2)
        t0 += n
    assert t0 == spec.shape[0]
    torch.cuda.synchronize()
    return sum_d.cpu().numpy(), sum_d2.cpu().numpy()


def _loop(be, spec, S, direct, kind, T):
    """The independent device path (CrossSpectra.jackknife_hip without `fused`): per trial the CSD kernel, its
    finalisation, the leave-one-out average in complex64, K5, minus direct, summed in float64."""
    _, K, F, C = spec.shape
    s, Sd, dd = _dev(spec), _dev(S), _dev(direct)
    sum_d, sum_d2 = _sums(F, C, kind)
    St = torch.empty_like(Sd)
    for t in range(spec.shape[0]):
        St.zero_()
        be.csd_accumulate(s[t].contiguous(), St)
        be.csd_finalize(St, 1.0 / K)
        loo = T * Sd - St
        loo /= T - 1
        d = (be.coh_normalize(loo, kind) - dd).to(sum_d.dtype)
        sum_d += d
        sum_d2 += (d.real ** 2 + d.imag ** 2) if kind == "complex" else d * d
    torch.cuda.synchronize()
    return sum_d.cpu().numpy(), sum_d2.cpu().numpy()


@pytest.mark.parametrize("case", JO.JACK_CASES, ids=JO.case_id)
def test_jack_coh_dispatch_edges(be, case):
    """K9 at the shapes of jack_oracle.JACK_CASES: both staging paths, frequency counts around the 8-XCD mapping, one
    to five tile rows, launches of one trial, all eight kinds; model bound and exact mirror."""
    kind, split = case[4], case[5]
    spec, S, direct, m = JO.case_data(case)
    sum_d, sum_d2 = _fused(be, spec, S, direct, kind, spec.shape[0], split)
    JO.check(sum_d, sum_d2, m, kind, "K9 device " + JO.case_id(case))


@pytest.mark.parametrize("case", [c for c in JO.JACK_CASES if c[:5] in ((33, 9, 5, 17, "imag"), (65, 7, 4, 16, "complex"))],
                         ids=JO.case_id)
def test_jack_coh_against_replicate_loop(be, case):
    """K9 and the replicate loop it replaces both meet the model's bound; the loop's err/tol is the yardstick the
    fused kernel's is read against."""
    kind, split = case[4], case[5]
    spec, S, direct, m = JO.case_data(case)
    T = spec.shape[0]
    fused = JO.err_over_tol(*_fused(be, spec, S, direct, kind, T, split), m)
    loop = JO.err_over_tol(*_loop(be, spec, S, direct, kind, T), m)
    print(f"K9 {JO.case_id(case)}: err/tol (sum_d, sum_d2) fused {fused[0]:.3f} {fused[1]:.3f}, "
          f"replicate loop {loop[0]:.3f} {loop[1]:.3f}")
    assert max(fused) <= 1.0 and max(loop) <= 1.0, (fused, loop)


def test_jack_coh_64_tapers(be):
    """64 tapers = 64 KiB of staging: the most the floor of the context's LDS limit allows."""
    case = (33, 2, 3, 64, "abs", [3])
    spec, S, direct, m = JO.case_data(case)
    sum_d, sum_d2 = _fused(be, spec, S, direct, "abs", 3, [3])
    JO.check(sum_d, sum_d2, m, "abs", "K9 device " + JO.case_id(case))


def _ppc_spectra(C, F, T, K):
    """The spectra of test_emu_kernels.test_ppc_kernel: a component common to all trials, the last channel all zero."""
    rng = np.random.default_rng(C)
    spec = (rng.normal(size=(T, K, F, C)) + 1j * rng.normal(size=(T, K, F, C))).astype(np.complex64)
    spec += (2.0 * rng.normal(size=(1, K, F, C))).astype(np.complex64)
    spec[..., C - 1] = 0
    return spec


@pytest.mark.parametrize("C,F,T,K", JO.PPC_EDGE_CASES + [(33, 2, 3, 64)])
def test_ppc_dispatch_edges(be, C, F, T, K):
    """K7 at its dispatch edges (more than 16 tapers, tile edges, four tile rows, frequencies around the 8-XCD mapping,
    a first launch of one trial, 64 tapers = the 64 KiB floor) against the oracle's walk over all trial pairs."""
    spec = _ppc_spectra(C, F, T, K)
    ref = O.ppc(O.spectral_dyadic_product(spec))[0]
    s = _dev(spec)
    U = torch.zeros((F, C, C), dtype=torch.complex64, device="cuda")
    be.ppc_accumulate(s[:1].reshape(-1, F, C).contiguous(), K, U)
    be.ppc_accumulate(s[1:].reshape(-1, F, C).contiguous(), K, U)
    got = be.ppc_finalize(U, T, lower_only=True).cpu().numpy()
    print(f"ppc device {C}-{F}-{T}-{K}: err/tol {excess(got, ref, rtol=1e-4, atol_rel=2e-5):.3f}")
    assert_parity(got, ref, what="ppc", rtol=1e-4, atol_rel=2e-5)
    assert np.array_equal(got, got.transpose(0, 2, 1)) and np.allclose(got[:, C - 1], 1, atol=1e-6)


@pytest.mark.parametrize("shape", [(1, 255), (1, 16, 16), (257,)], ids=lambda s: "x".join(map(str, s)))
def test_ppc_accumulate_csd_block_edges(be, shape):
    """ppc_accumulate_csd with 255 / 256 / 257 elements (one block short, full, and one thread into the second), five
    trials in launches of 1 + 4, against a float64 sum of s/|s| (an exact zero counts as 1).  Bound T * 4 * 2^-24 per
    component: the float32 sum of T unit phasors, each good to about 2 ulp by the rcp and rsq it is made with.  The
    moduli span 30 decades, inside the normal float32 range of both |s| and 1/|s|."""
    T = 5
    rng = np.random.default_rng(int(np.prod(shape)))
    csd = (rng.normal(size=(T,) + shape) + 1j * rng.normal(size=(T,) + shape)) * 10.0 ** rng.uniform(-15, 15, size=(T,) + shape)
    csd = csd.astype(np.complex64)
    csd.reshape(T, -1)[:, 3] = 0
    csd.reshape(T, -1)[2, -1] = 0
    z = csd.astype(np.complex128)
    mod = np.abs(z)
    ref = np.where(mod > 0, z / np.where(mod > 0, mod, 1.0), 1.0).sum(axis=0)
    c = _dev(csd)
    acc = torch.zeros(shape, dtype=torch.complex64, device="cuda")
    be.ppc_accumulate_csd(c[:1].contiguous(), acc)
    be.ppc_accumulate_csd(c[1:].contiguous(), acc)
    got = acc.cpu().numpy().astype(np.complex128)
    tol = T * 4 * 2.0 ** -24
    err = max(np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max())
    print(f"ppc_accumulate_csd {shape}: err/tol {err / tol:.3f}")
    assert err <= tol, err / tol
    assert got.reshape(-1)[3] == T


def test_ppc_finalize_rectangle(be):
    """ppc_finalize on a rectangular (F, ni, nj) accumulator: every element from its own phasor sum."""
    T = 7
    rng = np.random.default_rng(335)
    U = (rng.normal(size=(3, 3, 5)) + 1j * rng.normal(size=(3, 3, 5))).astype(np.complex64) * np.float32(2.0)
    ref = (np.abs(U.astype(np.complex128)) ** 2 - T) / (T * (T - 1))
    got = be.ppc_finalize(_dev(U), T, lower_only=False).cpu().numpy()
    print(f"ppc_finalize (3, 3, 5): err/tol {excess(got, ref):.3f}")
    assert_parity(got, ref, what="ppc_finalize on a rectangle")


def test_refusals_leave_the_sums_alone(be):
    """What the launchers refuse raises SpyHipError before anything is launched: accumulator and sums bit-identical.
    161 tapers are 164 864 B of staging, more than any LDS limit the context can hold."""
    rng = np.random.default_rng(161)
    F, C, K = 1, 3, 161
    spec = _dev((rng.normal(size=(K, F, C)) + 1j * rng.normal(size=(K, F, C))).astype(np.complex64))
    acc0 = (rng.normal(size=(F, C, C)) + 1j * rng.normal(size=(F, C, C))).astype(np.complex64)
    acc = _dev(acc0)
    with pytest.raises(be.SpyHipError):
        be.ppc_accumulate(spec, K, acc)
    assert np.array_equal(acc.cpu().numpy(), acc0)

    S, direct = _dev(acc0), _dev(np.abs(acc0).astype(np.float32))
    d0, d20 = rng.normal(size=(F, C, C)), rng.normal(size=(F, C, C))
    sum_d, sum_d2 = _dev(d0), _dev(d20)
    with pytest.raises(be.SpyHipError):
        be.jack_coh_accumulate(spec, K, S, direct, "abs", 4, sum_d, sum_d2)
    with pytest.raises(be.SpyHipError):                            # a jackknife of one trial has no replicate
        be.jack_coh_accumulate(spec[:3].contiguous(), 3, S, direct, "abs", 1, sum_d, sum_d2)
    assert np.array_equal(sum_d.cpu().numpy(), d0) and np.array_equal(sum_d2.cpu().numpy(), d20)

    rect = _dev((rng.normal(size=(2, 3, 5)) + 1j * rng.normal(size=(2, 3, 5))).astype(np.complex64))
    keep = rect.cpu().numpy()
    with pytest.raises(be.SpyHipError):                            # a lower-triangle accumulator is square
        be.ppc_finalize(rect, 4, lower_only=True)
    with pytest.raises(be.SpyHipError):                            # ppc needs a pair of trials
        be.ppc_finalize(rect, 1, lower_only=False)
    assert np.array_equal(rect.cpu().numpy(), keep)


@pytest.fixture(scope="module")
def coupled_data():
    """5 trials of 1 s at 1 kHz, 33 channels: a common broadband signal, 0 ... 3 samples late from channel to channel
    (coherences around 0.85, phases within 0.6 rad at 28 Hz: 'angle' is a stable quantity)."""
    rng = np.random.default_rng(1933)
    ntr, n, C = 5, 1000, 33
    common = rng.normal(size=ntr * n + 3)
    x = 0.6 * rng.normal(size=(ntr * n, C))
    for c in range(C):
        x[:, c] += 1.5 * common[3 - c % 4:3 - c % 4 + ntr * n]
    trl = np.stack([np.arange(ntr) * n, np.arange(1, ntr + 1) * n, np.zeros(ntr)], axis=1)
    return spy.AnalogData(x.astype(np.float32), samplerate=1000.0, trialdefinition=trl), ntr


@pytest.mark.parametrize("output", ["abs", "angle", "complex"])
def test_jackknife_end_to_end_19_tapers(be, coupled_data, monkeypatch, output):
    """connectivityanalysis(jackknife=True) with tapsmofrq=10 on 1 s of data: 19 tapers, K9's generic staging walk,
    9 frequencies; against the oracle-bound sequential engine under parity.jackknife_tolerances."""
    data, ntr = coupled_data
    launches = []
    inner = be.jack_coh_accumulate

    def watched(spec, ntaper, *a):
        launches.append(int(ntaper))
        return inner(spec, ntaper, *a)

    monkeypatch.setattr(be, "jack_coh_accumulate", watched)
    kw = dict(method="coh", tapsmofrq=10, jackknife=True, foilim=[20, 28], output=output)
    got = spy.connectivityanalysis(data, **kw)
    ref = spy.connectivityanalysis(data, **kw, compute_method="sequential", routine_classes=ORACLE_CONN)
    assert launches and all(k == 19 for k in launches), launches          # the fused path, more than 16 tapers
    assert got.data.shape == ref.data.shape and got.data.dtype == ref.data.dtype and got.data.shape[1] == 9
    cd = np.complex128 if output == "complex" else np.float64
    e = excess(got.data, ref.data)
    tol_var, tol_bias = jackknife_tolerances(ref.data, ref.jack_var, T=ntr)
    ev = np.abs(np.asarray(got.jack_var, dtype=np.float64) - ref.jack_var) / tol_var
    eb = np.abs(np.asarray(got.jack_bias, dtype=cd) - ref.jack_bias) / (1e-5 * np.abs(ref.jack_bias) + tol_bias)
    print(f"jackknife end to end, 19 tapers, {output}: err/tol estimate {e:.3f} var {ev.max():.3f} bias {eb.max():.3f}")
    assert e <= 1.0 and ev.max() <= 1.0 and eb.max() <= 1.0, (output, e, float(ev.max()), float(eb.max()))
