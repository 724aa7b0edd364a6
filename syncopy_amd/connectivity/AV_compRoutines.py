"""Compute functions on trial averages (signatures of syncopy/connectivity/AV_compRoutines.py:
normalize_csd_cF:36 / NormalizeCrossSpectra:115, granger_cF:293 / GrangerCausality:415)."""
import numpy as np
import torch

from .. import backend, parallel
from ..shared.computational_routine import ComputationalRoutine
from ..shared.const_def import spectralDTypes
from ..shared.errors import SPYValueError


def normalize_csd_cF(csd_av_dat, output="abs", chunkShape=None, noCompute=False):
    """Coherency C_ij = S_ij / sqrt(S_ii S_jj) of the trial-averaged CSD (nTime, nFreq, N, N)."""
    outShape = csd_av_dat.shape
    fmt = spectralDTypes["fourier"] if output in ("complex", "fourier") else spectralDTypes["abs"]
    if noCompute:
        return outShape, fmt
    backend.require_gpu()
    dev = torch.from_numpy(np.ascontiguousarray(csd_av_dat, dtype=np.complex64)).cuda()
    res = [backend.coh_normalize(dev[t], output) for t in range(dev.shape[0])]
    return backend.to_host(torch.stack(res, dim=0))


def phase_lag(st_csd, measure):
    """'ppc' | 'plv' | 'pli' | 'wpli' | 'wpli_debiased' of kept single-trial cross spectra (T, F, Ni, Nj) complex64 ->
    (1, F, Ni, Nj) float32 (all but the first not in the reference): the sums over trials of the batched path
    (backend.phase_accumulator), taken element by element, then its finalizer on the rectangle."""
    backend.require_gpu()
    st_csd = np.asarray(st_csd)
    T = st_csd.shape[0]
    acc, _, accumulate_csd, finalize = backend.phase_accumulator(measure, st_csd.shape[1:], "cuda")
    per = max(1, int((1 << 30) // max(1, int(np.prod(st_csd.shape[1:])) * 8)))
    for t0 in range(0, T, per):
        dev = torch.from_numpy(np.ascontiguousarray(st_csd[t0:t0 + per], dtype=np.complex64)).cuda()
        accumulate_csd(dev, acc)
    return backend.to_host(finalize(acc, T, lower_only=False))[np.newaxis]


def pairwise_phase_consistency(st_csd):
    """PPC of kept single-trial cross spectra (T, F, Ni, Nj) complex64 -> (1, F, Ni, Nj) float32: what the loop over
    PPC_column routines and its weighted average amount to (connectivity_analysis.py:624-663;
    ST_compRoutines.py:159-233), through K7's closed form - unit phasors summed over trials, then
    (|U|^2 - T)/(T(T-1))."""
    return phase_lag(st_csd, "ppc")


class _AverageRoutine(ComputationalRoutine):
    dimord = ["time", "freq", "channel_i", "channel_j"]

    def pre_check(self):
        if self.numTrials is None:
            raise SPYValueError("Initialize the computational Routine first!", varname=self.__class__.__name__,
                                actual="ComputationalRoutine not initialized!")
        if self.numTrials != 1:
            raise SPYValueError("1 trial: normalizations can only be done on averaged quantities!", varname="data",
                                actual=f"DataSet contains {self.numTrials} trials")

    def _device_input(self, data):
        dev = getattr(data, "_dev", None)
        if dev is None:
            dev = torch.from_numpy(np.ascontiguousarray(data.data, dtype=np.complex64)).cuda()
        return dev

    @staticmethod
    def _keep_on_device(out, res, fetch=None):
        """`res` is the result and stays in HBM until somebody reads `.data` (then one pinned, chunked copy, or `fetch`): a
        chained analysis or a plot of a few channel pairs never pays for the whole array (0.5 GB of coherence)."""
        out._dev = res
        out.set_pending(fetch or (lambda: backend.to_host(res)), tuple(res.shape),
                        np.complex64 if res.is_complex() else np.float32)

    def process_metadata(self, data, out):
        out.channel_i = np.array(data.channel_i)
        out.channel_j = np.array(data.channel_j)
        out.freq = data.freq
        out.trialdefinition = data.trialdefinition.copy()
        out.samplerate = data.samplerate


class NormalizeCrossSpectra(_AverageRoutine):
    computeFunction = staticmethod(normalize_csd_cF)
    method = ""
    valid_kws = ["output"]

    def evaluate_device(self, csd):
        """AV stage on one device CSD (F, C, C) -> (F, C, C); used by the streaming jackknife."""
        return backend.coh_normalize(csd.contiguous(), self.cfg["output"])

    def jackknife_accumulate(self, spec, ntaper, csd, direct, ntrials_total, sum_d, sum_d2):
        """Pass 2 of the streaming jackknife for a batch of trials in ONE kernel (K9): single-trial cross spectra,
        leave-one-out averages, their coherence and the sums of d_t / |d_t|^2 never leave the registers."""
        backend.jack_coh_accumulate(spec, ntaper, csd.contiguous(), direct.contiguous(), self.cfg["output"],
                                    ntrials_total, sum_d, sum_d2)

    def compute_hip(self, data, out):
        raw = getattr(data, "_acc_raw", None)
        events = getattr(raw, "spyhip_range_events", None) if raw is not None else None
        if events:
            # the ST stage's last update came frequency range by frequency range: normalise and ship each range to a
            # page-locked landing block while the next is still being accumulated (backend.coh_pipeline) - reading
            # `.data` then waits for the copy of the last range only (compute_sequential hands over a result the caller
            # can read, computational_routine.py:1022-1036)
            res, landing = backend.coh_pipeline(raw, data._acc_scale, self.cfg["output"], events)
            res = res.unsqueeze(0)
            shape = tuple(res.shape)
            self._keep_on_device(out, res, (lambda: landing.array().reshape(shape)) if landing is not None else None)
            return
        if raw is not None:
            # straight from the ST stage's raw accumulator: scale + normalise + convert + mirror in one pass
            self._keep_on_device(out, backend.coh_from_accumulator(raw, data._acc_scale, self.cfg["output"]).unsqueeze(0))
            return
        dev = self._device_input(data)
        res = torch.stack([backend.coh_normalize(dev[t].contiguous(), self.cfg["output"])
                           for t in range(dev.shape[0])], dim=0)
        out._dev = res
        out.data = backend.to_host(res)


def phaseslope_cF(csd_av_dat, half=0, chunkShape=None, noCompute=False):
    """Phase slope index (Nolte et al. 2008, FieldTrip's `psi`; not in the reference) of the trial-averaged CSD
    (nTime, nFreq, N, N): per time sample the sum over the 2 * half edges around each bin of Im(conj(c(f)) c(f + 1)), c the
    coherency, as float32 (nTime, nFreq, N, N) [sender, receiver] with whole planes NaN where the band does not fit;
    half = 0: the sum over the whole axis, (nTime, 1, N, N)."""
    outShape = (csd_av_dat.shape[0], csd_av_dat.shape[1] if half else 1) + tuple(csd_av_dat.shape[2:])
    if noCompute:
        return outShape, spectralDTypes["abs"]
    backend.require_gpu()
    dev = torch.from_numpy(np.ascontiguousarray(csd_av_dat, dtype=np.complex64)).cuda()
    res = [backend.phase_slope(dev[t], half) for t in range(dev.shape[0])]
    return backend.to_host(torch.stack(res, dim=0))


class PhaseSlope(_AverageRoutine):
    """AV stage of method 'psi' (K13)."""
    computeFunction = staticmethod(phaseslope_cF)
    method = ""
    valid_kws = ["half"]

    def evaluate_device(self, csd):
        """AV stage on one device CSD (F, C, C) -> (F or 1, C, C) float32; used by the streaming jackknife, one launch per
        replicate."""
        return backend.phase_slope(csd.contiguous(), self.cfg["half"])

    def compute_hip(self, data, out):
        raw = getattr(data, "_acc_raw", None)
        if raw is not None:
            # straight from the ST stage's raw accumulator.  One launch: a band couples neighbouring frequency ranges, so an
            # accumulator that arrived range by range is waited for as a whole
            stream = torch.cuda.current_stream(raw.device)
            for _, _, ev in getattr(raw, "spyhip_range_events", None) or ():
                stream.wait_event(ev)
            self._keep_on_device(out, backend.phase_slope_from_accumulator(raw, data._acc_scale, self.cfg["half"]).unsqueeze(0))
            return
        dev = self._device_input(data)
        self._keep_on_device(out, torch.stack([backend.phase_slope(dev[t].contiguous(), self.cfg["half"])
                                               for t in range(dev.shape[0])], dim=0))

    def process_metadata(self, data, out):
        super().process_metadata(data, out)
        if not self.cfg["half"]:
            out.freq = np.array([np.mean(data.freq)])


def granger_cF(csd_av_dat, rtol=5e-6, nIter=100, cond_max=1e4, chunkShape=None, noCompute=False):
    """Pairwise Granger-Geweke causality from the trial-averaged CSD (1, nFreq, N, N): regularisation,
    Wilson factorisation and the Granger formula all run on the device.  Returns (1, nFreq, N, N) float32
    and the reference's metadata keys (AV_compRoutines.py:404-409)."""
    outShape = csd_av_dat.shape
    if noCompute:
        return outShape, spectralDTypes["abs"]
    backend.require_gpu()
    dev = torch.from_numpy(np.ascontiguousarray(csd_av_dat[0], dtype=np.complex64)).cuda()
    G, meta = backend.granger(dev, rtol=rtol, niter=nIter, cond_max=cond_max, eps_max=1e-1)
    return backend.to_host(G)[None, ...], _granger_metadata(meta)


def _granger_metadata(meta):
    return {
        "converged--bool": np.array(meta["converged"]),
        "max rel. err--float": np.array(meta["max rel. err"]),
        "reg. factor--float": np.array(meta["reg. factor"]),
        "initial cond. num--float": np.array(meta["initial cond. num"]),
    }


class _WilsonRoutine(_AverageRoutine):
    """AV stages on the Wilson factorisation of a trial-averaged CSD.  A subclass supplies `_of_plane(csd)`: one device
    CSD (F, C, C) every rank holds -> (its measure (F, C, C) float32, the factorisation's metadata)."""
    method = ""
    metadata_keys = ("converged", "max rel. err", "reg. factor", "initial cond. num")

    def compute_hip(self, data, out):
        dev = self._device_input(data)
        res, self.metadata = [], []
        for t in range(dev.shape[0]):            # one trial average, or the jackknife's leave-one-out replicates
            plane, meta = self._of_plane(dev[t].contiguous())
            res.append(plane)
            self.metadata.append(_granger_metadata(meta))
        out._dev = torch.stack(res, dim=0)
        out.data = backend.to_host(out._dev)

    def process_metadata(self, data, out):
        super().process_metadata(data, out)
        for key, value in (self.metadata[0] or {}).items():
            label, cast = key.split("--")
            out.info[label] = bool(value) if cast == "bool" else float(value)


class GrangerCausality(_WilsonRoutine):
    computeFunction = staticmethod(granger_cF)
    valid_kws = ["rtol", "nIter", "cond_max"]

    def evaluate_device(self, csd):
        """AV stage on one device CSD (F, C, C) -> Granger (F, C, C) float32; keeps the metadata of the first call
        (the direct estimate) for `out.info`."""
        if not self.metadata:                    # the direct estimate: every rank calls with the same CSD
            G, meta = self._granger(csd.contiguous())
            self.metadata = [_granger_metadata(meta)]
            return G
        # jackknife replicates belong to the rank that owns the left-out trial: no collective here
        return backend.granger(csd.contiguous(), rtol=self.cfg["rtol"], niter=self.cfg["nIter"],
                               cond_max=self.cfg["cond_max"], eps_max=1e-1)[0]

    def _granger(self, csd):
        """One trial-averaged CSD every rank holds -> Granger values on every rank.  With a process group the
        frequencies are sharded over the ranks (wilson_sharded.py); otherwise one spyhip_granger call."""
        kw = dict(rtol=self.cfg["rtol"], niter=self.cfg["nIter"], cond_max=self.cfg["cond_max"], eps_max=1e-1)
        if parallel.collective_active():
            from .wilson_sharded import granger_hip_sharded
            return granger_hip_sharded(csd, **kw)
        return backend.granger(csd, **kw)

    _of_plane = _granger


def directed_cF(csd_av_dat, method="dtf", noise_weighted=False, output="abs", rtol=5e-6, nIter=100, cond_max=1e4,
                chunkShape=None, noCompute=False):
    """Directed transfer function ('dtf') or partial directed coherence ('pdc') from the trial-averaged CSD
    (1, nFreq, N, N), not in the reference: the regularisation and Wilson factorisation of granger_cF, then
    |H| normalised over the senders of a receiver (dtf) or |H^-1| over the receivers of a sender (pdc), weighted with
    the noise variances for `noise_weighted` (directed coherence / generalised PDC); output 'pow' squares.  Returns
    (1, nFreq, N, N) float32 [sender, receiver] and granger_cF's metadata keys."""
    outShape = csd_av_dat.shape
    if noCompute:
        return outShape, spectralDTypes["abs"]
    backend.require_gpu()
    dev = torch.from_numpy(np.ascontiguousarray(csd_av_dat[0], dtype=np.complex64)).cuda()
    res, meta = backend.directed(dev, method, noise_weighted=noise_weighted, squared=(output == "pow"), rtol=rtol,
                                 niter=nIter, cond_max=cond_max, eps_max=1e-1)
    return backend.to_host(res)[None, ...], _granger_metadata(meta)


class DirectedMeasure(_WilsonRoutine):
    """AV stage of method 'dtf' / 'pdc'.  Every rank of a process group factorises the whole CSD it holds: the
    frequency shards of GrangerCausality are not used here.  (No `evaluate_device`: there is no jackknife of these.)"""
    computeFunction = staticmethod(directed_cF)
    valid_kws = ["method", "noise_weighted", "output", "rtol", "nIter", "cond_max"]

    def _of_plane(self, csd):
        cfg = self.cfg
        return backend.directed(csd, cfg["method"], noise_weighted=cfg["noise_weighted"], squared=(cfg["output"] == "pow"),
                                rtol=cfg["rtol"], niter=cfg["nIter"], cond_max=cfg["cond_max"], eps_max=1e-1)


def normalize_ccov_cF(trl_av_dat, chunkShape=None, noCompute=False):
    """Cross-correlation from the trial-averaged cross-covariance (nLags, 1, N, N): divided by the square roots of
    the zero-lag auto-covariances (AV_compRoutines.py:166-228)."""
    outShape = trl_av_dat.shape
    if noCompute:
        return outShape, spectralDTypes["abs"]
    backend.require_gpu()
    dev = torch.from_numpy(np.ascontiguousarray(trl_av_dat, dtype=np.float32)).cuda()
    return backend.to_host(backend.ccov_normalize_(dev[:, 0].contiguous()))[:, np.newaxis]


class NormalizeCrossCov(_AverageRoutine):
    computeFunction = staticmethod(normalize_ccov_cF)
    method = ""
    valid_kws = []

    def compute_hip(self, data, out):
        dev = getattr(data, "_dev", None)
        if dev is None:
            dev = torch.from_numpy(np.ascontiguousarray(data.data, dtype=np.float32)).cuda()
        res = backend.ccov_normalize_(dev[:, 0].contiguous().clone()).unsqueeze(1)
        out._dev = res
        out.data = backend.to_host(res)
