"""NumPy + ctypes host of libspyhip.so - no PyTorch anywhere (the reference depends on NumPy/SciPy only,
pyproject.toml:28-29).  What a Syncopy maintainer would put behind `ComputationalRoutine.compute_hip`
(INTEGRATION.md): the library allocates HBM, holds the trial queue, runs the kernels, sums over ranks with RCCL and
hands back NumPy arrays.

    dev = abi.Device(0)
    q = dev.upload_trials(data, sampleinfo)                    # (rows x channels) float32 + trial row ranges -> HBM
    pow_ = dev.mtmfft(q, tapers, scale, nfft, output="pow", keeptapers=False)
    coh = dev.coherence(q, tapers, scale, nfft, output="abs")

The PyTorch-backed front ends (`spy.freqanalysis`, `spy.connectivityanalysis`) call the very same entry points with
tensor pointers; nothing here is a second implementation of any arithmetic.

A process that really is NumPy-only sets SPY_NO_TORCH=1 before the first use: otherwise `_lib.load()` imports an
installed torch FIRST, so that a later `import torch` in the same process does not bind to the system libamdhip64 this
library brings in (same SONAME as the runtime bundled with the torch wheel).

`reference_mean` (the per-channel mean in the reference's float32 summation order, K0) reproduces NumPy bit for bit
for dimord time x channel; for channel x time data the reference averages a transposed view with pairwise summation
and the result agrees to float32 rounding only.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SpyHipError, check  # noqa: F401

OUTPUT_KIND = {"pow": 0, "abs": 1, "fourier": 2, "complex": 2, "real": 3, "imag": 4, "angle": 5,
               "absreal": 6, "absimag": 7}
DETREND = {None: -1, False: -1, 0: 0, 1: 1}
PHASELAG_MEASURE = {"pli": 0, "wpli": 1, "wpli_debiased": 2}       # SPYHIP_PHASELAG_* (include/spyhip.h)
ENVCORR_MEASURE = {"amplcorr": 0, "powcorr": 1, "powcorr_ortho": 2}  # SPYHIP_ENVCORR_*


class Buffer:
    """A block of HBM owned by the library (spyhip_alloc / spyhip_free)."""

    def __init__(self, dev, shape, dtype, zero=False):
        self.dev, self.shape, self.dtype = dev, tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(dev.lib.spyhip_alloc(dev.handle, self.nbytes, C.byref(p)), "spyhip_alloc")
        self.ptr = p
        if zero:
            check(dev.lib.spyhip_memset(dev.handle, self.ptr, 0, self.nbytes), "spyhip_memset")

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(self.dev.lib.spyhip_download(self.dev.handle, out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes),
              "spyhip_download")
        return out

    def free(self):
        if self.ptr is not None and self.ptr.value:
            self.dev.lib.spyhip_free(self.dev.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class TrialQueue:
    """spyhip_queue: the (rows x channels) float32 matrix of an AnalogData object in HBM with its trials' row
    ranges (`sampleinfo`, datatype/base_data.py:993) - uploaded once, indexed exactly."""

    def __init__(self, dev, data, sampleinfo):
        data = np.ascontiguousarray(data, dtype=np.float32)
        si = np.ascontiguousarray(sampleinfo, dtype=np.int64)
        if data.ndim != 2 or si.ndim != 2 or si.shape[1] != 2:
            raise ValueError("data must be (rows, channels), sampleinfo (trials, 2)")
        self.dev = dev
        self.nrows, self.nchan = data.shape
        self.ntrials = si.shape[0]
        self.lengths = (si[:, 1] - si[:, 0]).astype(np.int64)
        h = C.c_void_p()
        check(dev.lib.spyhip_queue_upload(dev.handle, data.ctypes.data_as(C.c_void_p), self.nrows, self.nchan,
                                          si.ctypes.data_as(_lib.c_i64p), self.ntrials, C.byref(h)),
              "spyhip_queue_upload")
        self.handle = h
        self.data_d = C.c_void_p(dev.lib.spyhip_queue_data(h))
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int()
        check(dev.lib.spyhip_queue_segments(h, C.byref(a), C.byref(b), C.byref(n)), "spyhip_queue_segments")
        self.start_d, self.stop_d = a, b

    def free(self):
        if self.handle is not None:
            self.dev.lib.spyhip_queue_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Device:
    """One spyhip_ctx; every call is complete when it returns a NumPy array."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.spyhip_ctx_create(int(device), C.byref(h)), "spyhip_ctx_create")
        self.handle = h
        self.rank, self.nranks = 0, 1

    # ---- data
    def upload_trials(self, data, sampleinfo):
        return TrialQueue(self, data, sampleinfo)

    def synchronize(self):
        check(self.lib.spyhip_ctx_synchronize(self.handle), "spyhip_ctx_synchronize")

    # ---- ranks (RCCL inside the library; the 128-byte id travels by whatever means the host has)
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        check(self.lib.spyhip_comm_unique_id(buf), "spyhip_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        check(self.lib.spyhip_comm_init(self.handle, C.c_char_p(unique_id), int(rank), int(nranks)), "spyhip_comm_init")
        self.rank, self.nranks = int(rank), int(nranks)

    def comm_destroy(self):
        check(self.lib.spyhip_comm_destroy(self.handle), "spyhip_comm_destroy")
        self.rank, self.nranks = 0, 1

    @property
    def has_comm(self):
        return self.lib.spyhip_comm_info(self.handle, None, None) == 0

    # ---- K1
    def _plan(self, nsig, nfft, nchan, tapers, scale, detrend, demean_taper, freq_idx, output, keeptapers):
        tapers = np.ascontiguousarray(np.atleast_2d(tapers), dtype=np.float64)
        assert tapers.shape[1] == nsig
        fi = None if freq_idx is None else np.ascontiguousarray(freq_idx, dtype=np.int32)
        nfsel = nfft // 2 + 1 if fi is None else int(fi.size)
        h = C.c_void_p()
        check(self.lib.spyhip_fft_plan_create(
            self.handle, int(nsig), int(nfft), int(nchan), tapers.shape[0], tapers.ctypes.data_as(_lib.c_f64p),
            float(scale), DETREND[detrend], int(bool(demean_taper)),
            None if fi is None else fi.ctypes.data_as(_lib.c_i32p), nfsel, OUTPUT_KIND[output], int(bool(keeptapers)),
            C.byref(h)), "spyhip_fft_plan_create")
        if DETREND[detrend] == 0:      # whole trials: the reference's float32 row-order mean (compRoutines.py:169-170)
            check(self.lib.spyhip_fft_plan_set_reference_mean(h, 1), "spyhip_fft_plan_set_reference_mean")
        return h, tapers.shape[0], nfsel

    def mtmfft(self, queue, tapers, scale, nfft=None, detrend=0, demean_taper=False, freq_idx=None, output="pow",
               keeptapers=False, device_result=False):
        """mtmfft_cF for all trials of the queue (equal length): (T, Kout, F', C) float32 / complex64."""
        nsig = int(queue.lengths[0])
        if np.any(queue.lengths != nsig):
            raise ValueError("one call serves trials of one length (group them by length)")
        nfft = nsig if nfft is None else int(nfft)
        plan, K, nfsel = self._plan(nsig, nfft, queue.nchan, tapers, scale, detrend, demean_taper, freq_idx, output,
                                    keeptapers)
        try:
            kout = K if keeptapers else 1
            out = Buffer(self, (queue.ntrials, kout, nfsel, queue.nchan),
                         np.complex64 if OUTPUT_KIND[output] == 2 else np.float32)
            check(self.lib.spyhip_fft_exec(plan, queue.data_d, queue.nchan, None, queue.start_d, queue.start_d,
                                           queue.stop_d, queue.ntrials, out.ptr), "spyhip_fft_exec")
            if device_result:
                self.synchronize()
                return out
            res = out.numpy()
            out.free()
            return res
        finally:
            self.synchronize()
            self.lib.spyhip_fft_plan_destroy(plan)

    # ---- K1 + K4 (+ C1) + K5
    def csd_accumulator(self, queue, tapers, scale, nfft=None, detrend=0, demean_taper=False, batch_bytes=8 << 30):
        """Raw lower-triangle accumulator sum_t sum_k X X^H of this rank's trials, summed over ranks if a
        communicator exists: (Buffer (F, C, C) complex64, number of tapers)."""
        spec = self.mtmfft(queue, tapers, scale, nfft, detrend, demean_taper, None, "fourier", True,
                           device_result=True)
        T, K, F, Cn = spec.shape
        acc = Buffer(self, (F, Cn, Cn), np.complex64, zero=True)
        check(self.lib.spyhip_csd_accumulate(self.handle, spec.ptr, T * K, F, Cn, acc.ptr), "spyhip_csd_accumulate")
        self.synchronize()
        spec.free()
        if self.has_comm:
            check(self.lib.spyhip_allreduce_csd(self.handle, acc.ptr, F, Cn), "spyhip_allreduce_csd")
        return acc, K

    def csd(self, queue, tapers, scale, nfft=None, detrend=0, demean_taper=False, ntrials_total=None):
        """Trial-averaged cross-spectral density (F, C, C) complex64 (cross_spectra_cF + trial mean)."""
        acc, K = self.csd_accumulator(queue, tapers, scale, nfft, detrend, demean_taper)
        T = queue.ntrials if ntrials_total is None else int(ntrials_total)
        F, Cn, _ = acc.shape
        check(self.lib.spyhip_csd_finalize(self.handle, acc.ptr, F, Cn, 1.0 / (K * T)), "spyhip_csd_finalize")
        res = acc.numpy()
        acc.free()
        return res

    def coherence(self, queue, tapers, scale, nfft=None, detrend=0, output="abs", ntrials_total=None):
        """connectivityanalysis(method='coh'): (F, C, C) float32 (complex64 for output='complex')."""
        acc, K = self.csd_accumulator(queue, tapers, scale, nfft, detrend, False)
        T = queue.ntrials if ntrials_total is None else int(ntrials_total)
        F, Cn, _ = acc.shape
        kind = OUTPUT_KIND[output]
        out = Buffer(self, (F, Cn, Cn), np.complex64 if kind == 2 else np.float32)
        check(self.lib.spyhip_coh_from_accumulator(self.handle, acc.ptr, F, Cn, 1.0 / (K * T), kind, out.ptr),
              "spyhip_coh_from_accumulator")
        res = out.numpy()
        out.free()
        acc.free()
        return res

    # ---- K1 + K4 (+ C1) + K13
    def phase_slope(self, queue, tapers, scale, nfft=None, detrend=0, half=0, ntrials_total=None):
        """connectivityanalysis(method='psi'): (F, C, C) float32 [f, sender, receiver] for the half width `half` >= 1 in
        bins, whole planes NaN where the band does not fit; half = 0: the whole axis, (1, C, C)."""
        acc, K = self.csd_accumulator(queue, tapers, scale, nfft, detrend, False)
        T = queue.ntrials if ntrials_total is None else int(ntrials_total)
        F, Cn, _ = acc.shape
        out = Buffer(self, (F if half else 1, Cn, Cn), np.float32)
        try:
            check(self.lib.spyhip_phaseslope_from_accumulator(self.handle, acc.ptr, F, Cn, 1.0 / (K * T), int(half), out.ptr),
                  "spyhip_phaseslope_from_accumulator")
            return out.numpy()
        finally:
            out.free()
            acc.free()

    # ---- K1 + K7 / K10
    def phase_measure(self, queue, tapers, scale, nfft=None, detrend=0, method="wpli", ntrials_total=None):
        """connectivityanalysis(method='ppc' | 'plv' | 'pli' | 'wpli' | 'wpli_debiased'): (F, C, C) float32.  The sums
        over this rank's trials are summed over ranks if a communicator exists (`ntrials_total`: all ranks' trials)."""
        if method not in ("ppc", "plv") + tuple(PHASELAG_MEASURE):
            raise ValueError(f"no phase measure {method!r}")
        spec = self.mtmfft(queue, tapers, scale, nfft, detrend, False, None, "fourier", True, device_result=True)
        T, K, F, Cn = spec.shape
        phasors = method in ("ppc", "plv")
        acc = Buffer(self, (F, Cn, Cn, 2 if phasors else 4), np.float32, zero=True)
        accumulate = self.lib.spyhip_ppc_accumulate if phasors else self.lib.spyhip_phaselag_accumulate
        check(accumulate(self.handle, spec.ptr, T, K, F, Cn, acc.ptr), "spyhip_%s_accumulate" % ("ppc" if phasors else "phaselag"))
        self.synchronize()
        spec.free()
        if self.has_comm:
            check(self.lib.spyhip_allreduce(self.handle, acc.ptr, int(np.prod(acc.shape)), 0), "spyhip_allreduce")
        T = T if ntrials_total is None else int(ntrials_total)
        out = Buffer(self, (F, Cn, Cn), np.float32)
        if method == "ppc":
            check(self.lib.spyhip_ppc_finalize(self.handle, acc.ptr, F, Cn, Cn, 1, T, out.ptr), "spyhip_ppc_finalize")
        elif method == "plv":
            check(self.lib.spyhip_plv_finalize(self.handle, acc.ptr, F, Cn, Cn, 1, T, out.ptr), "spyhip_plv_finalize")
        else:
            check(self.lib.spyhip_phaselag_finalize(self.handle, acc.ptr, F, Cn, Cn, 1, T, PHASELAG_MEASURE[method], out.ptr),
                  "spyhip_phaselag_finalize")
        res = out.numpy()
        out.free()
        acc.free()
        return res

    # ---- directed measures of the Wilson factors
    def zinv(self, M):
        """np.linalg.inv of a stack of complex128 matrices (batch, n, n) with the Wilson stage's kernels (spyhip_zinv)."""
        M = np.ascontiguousarray(M, dtype=np.complex128)
        if M.ndim != 3 or M.shape[1] != M.shape[2]:
            raise ValueError("M must be (batch, n, n)")
        buf = self._put(M, np.complex128)
        try:
            check(self.lib.spyhip_zinv(self.handle, buf.ptr, buf.ptr, M.shape[0], M.shape[1]), "spyhip_zinv")
            return buf.numpy()
        finally:
            self.synchronize()
            buf.free()

    def directed_norm(self, M, w=None, axis=0, squared=False):
        """spyhip_directed_norm of complex128 `M` (F, n, n): float32 [f, sender, receiver], normalised along the rows
        (axis 0: DTF of M = H) or the columns (axis 1: PDC of M = H^-1) of M with the weights `w` (n, or None)."""
        M = np.ascontiguousarray(M, dtype=np.complex128)
        if M.ndim != 3 or M.shape[1] != M.shape[2]:
            raise ValueError("M must be (F, n, n)")
        F, n, _ = M.shape
        if w is not None and np.size(w) != n:
            raise ValueError("w must hold one weight per channel")
        md = self._put(M, np.complex128)
        wd = self._put(np.ravel(w), np.float64) if w is not None else None
        out = Buffer(self, (F, n, n), np.float32)
        try:
            check(self.lib.spyhip_directed_norm(self.handle, md.ptr, wd.ptr if wd is not None else None, F, n, int(axis),
                                                int(bool(squared)), out.ptr), "spyhip_directed_norm")
            return out.numpy()
        finally:
            self.synchronize()
            for b in (md, wd, out):
                if b is not None:
                    b.free()

    # ---- K1 + K12
    def envelope_measure(self, queue, tapers, scale, nfft=None, detrend=0, method="powcorr_ortho", nrep_total=None):
        """connectivityanalysis(method='amplcorr' | 'powcorr' | 'powcorr_ortho'): (F, C, C) float32.  The sums over the
        repetitions (trial x taper) of this rank's trials are summed over ranks if a communicator exists (`nrep_total`:
        all ranks' repetitions)."""
        if method not in ENVCORR_MEASURE:
            raise ValueError(f"no envelope measure {method!r}")
        spec = self.mtmfft(queue, tapers, scale, nfft, detrend, False, None, "fourier", True, device_result=True)
        T, K, F, Cn = spec.shape
        measure = ENVCORR_MEASURE[method]
        pair = Buffer(self, (5 if method == "powcorr_ortho" else 1, F, Cn, Cn), np.float64, zero=True)
        chan = Buffer(self, (F, Cn, 2), np.float64, zero=True)
        check(self.lib.spyhip_envcorr_accumulate(self.handle, spec.ptr, T, K, F, Cn, measure, pair.ptr, chan.ptr),
              "spyhip_envcorr_accumulate")
        self.synchronize()
        spec.free()
        if self.has_comm:
            for acc in (pair, chan):
                check(self.lib.spyhip_allreduce(self.handle, acc.ptr, int(np.prod(acc.shape)), 1), "spyhip_allreduce")
        nrep = T * K if nrep_total is None else int(nrep_total)
        out = Buffer(self, (F, Cn, Cn), np.float32)
        check(self.lib.spyhip_envcorr_finalize(self.handle, pair.ptr, chan.ptr, F, Cn, nrep, measure, out.ptr),
              "spyhip_envcorr_finalize")
        res = out.numpy()
        for b in (out, pair, chan):
            b.free()
        return res

    # ---- spy.timelockanalysis
    def cov(self, trials, ddof=None):
        """np.cov(trial, ddof=ddof, rowvar=False) of every trial of `trials` (T, n, channels) float32: (T, channels,
        channels) float32 (cov_cF; float64 arithmetic on the device, one rounding).  ddof=None is NumPy's default, 1."""
        x = np.ascontiguousarray(trials, dtype=np.float32)
        if x.ndim != 3:
            raise ValueError("trials must be (T, n, channels)")
        T, n, Cn = x.shape
        xd = Buffer(self, x.shape, np.float32)
        out = Buffer(self, (T, Cn, Cn), np.float32)
        try:
            check(self.lib.spyhip_upload(self.handle, xd.ptr, x.ctypes.data_as(C.c_void_p), x.nbytes), "spyhip_upload")
            check(self.lib.spyhip_cov_f32(self.handle, xd.ptr, out.ptr, T, n, Cn, 1 if ddof is None else int(ddof)),
                  "spyhip_cov_f32")
            return out.numpy()
        finally:
            self.synchronize()
            xd.free()
            out.free()

    # ---- spy.spike_psth
    def _put(self, arr, dtype):
        arr = np.ascontiguousarray(arr, dtype=dtype)
        buf = Buffer(self, arr.shape, dtype)
        if arr.nbytes:
            check(self.lib.spyhip_upload(self.handle, buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes),
                  "spyhip_upload")
        return buf

    def psth(self, spikes, trialdefinition, samplerate, edges, output="rate", channels=None, units=None):
        """Peristimulus time histograms (psth_cF for every trial): `spikes` (nSpikes, 3) integers [sample, channel, unit]
        sorted by sample, `trialdefinition` (T, 3) [start, end, onset] in samples, `edges` the float64 bin edges in
        seconds, `output` 'rate', 'spikecount' or 'proportion'; `channels` / `units`: the channel / unit numbers to keep
        (None: all).  Returns (hist (T, nbins, ncols) float32, columns (ncols, 2) int64): one column per (channel, unit)
        pair that occurs in the trials, sorted; NaN in the bins a trial does not reach (psth.py:133-155)."""
        from .statistics.spike_psth import column_tables, valid_bins
        spikes = np.asarray(spikes)
        trl = np.asarray(trialdefinition, dtype=np.float64)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        if spikes.ndim != 2 or spikes.shape[1] != 3 or trl.ndim != 2 or trl.shape[1] < 3 or edges.ndim != 1:
            raise ValueError("spikes must be (nSpikes, 3), trialdefinition (T, 3), edges one-dimensional")
        if output not in ("rate", "spikecount", "proportion") or edges.size < 2:
            raise ValueError("output is 'rate', 'spikecount' or 'proportion'; at least two edges")
        sample = np.ascontiguousarray(spikes[:, 0], dtype=np.int64)
        if spikes.shape[0] < 1 or np.any(np.diff(sample) < 0) or spikes[:, 1:].min() < 0 or spikes[:, 1:].max() >= 2 ** 31:
            raise ValueError("spikes sorted by sample, channel and unit numbers in [0, 2^31)")
        nchan, nunit = int(spikes[:, 1].max()) + 1, int(spikes[:, 2].max()) + 1
        chan_ok, unit_ok = np.zeros(nchan, np.uint8), np.zeros(nunit, np.uint8)
        chan_ok[slice(None) if channels is None else np.asarray(channels, dtype=np.int64)] = 1
        unit_ok[slice(None) if units is None else np.asarray(units, dtype=np.int64)] = 1
        T, nbins = trl.shape[0], edges.size - 1
        rows = np.searchsorted(sample, trl[:, :2].astype(np.int64).ravel()).reshape(T, 2).astype(np.int64)
        rows[:, 1] = np.maximum(rows[:, 1], rows[:, 0])
        lohi = np.array([valid_bins(edges, s, e, o, float(samplerate)) for s, e, o in trl[:, :3]],
                        dtype=np.int32).reshape(T, 2)
        bufs = []

        def put(arr, dtype):
            bufs.append(self._put(arr, dtype))
            return bufs[-1]
        try:
            sample_d, chan_d, unit_d = put(sample, np.int64), put(spikes[:, 1], np.int32), put(spikes[:, 2], np.int32)
            lo_d, hi_d = put(rows[:, 0], np.int64), put(rows[:, 1], np.int64)
            flags_d = Buffer(self, (nchan, nunit), np.uint8, zero=True)
            bufs.append(flags_d)
            check(self.lib.spyhip_psth_presence(self.handle, chan_d.ptr, unit_d.ptr, lo_d.ptr, hi_d.ptr, T,
                                                int((rows[:, 1] - rows[:, 0]).max(initial=0)), put(chan_ok, np.uint8).ptr,
                                                nchan, put(unit_ok, np.uint8).ptr, nunit, flags_d.ptr),
                  "spyhip_psth_presence")
            columns, lut, unit_k, col_k, nk = column_tables(flags_d.numpy())
            ncols = columns.shape[0]
            if ncols == 0 or T == 0:
                return np.zeros((T, nbins, ncols), dtype=np.float32), columns
            rows_d = Buffer(self, (T, nbins + 1), np.int64)
            out = Buffer(self, (T, nbins, ncols), np.float32)
            bufs += [rows_d, out]
            edges_d, lut_d = put(edges, np.float64), put(lut, np.int32)
            check(self.lib.spyhip_psth_bin_rows(self.handle, sample_d.ptr, lo_d.ptr, hi_d.ptr,
                                                put(trl[:, 0], np.int64).ptr, put(trl[:, 2], np.int64).ptr, T,
                                                edges_d.ptr, nbins + 1, float(samplerate), rows_d.ptr),
                  "spyhip_psth_bin_rows")
            scale = float(1 / np.diff(edges)[0]) if output == "rate" else 1.0
            check(self.lib.spyhip_psth_count(self.handle, chan_d.ptr, unit_d.ptr, rows_d.ptr, lut_d.ptr, nchan, nunit,
                                             put(lohi, np.int32).ptr, T, nbins, ncols, scale, out.ptr),
                  "spyhip_psth_count")
            if output == "proportion":
                work = Buffer(self, (T, nk), np.int32)
                bufs.append(work)
                check(self.lib.spyhip_psth_proportion(self.handle, chan_d.ptr, unit_d.ptr, lo_d.ptr, hi_d.ptr, rows_d.ptr,
                                                      lut_d.ptr, nchan, nunit, put(unit_k, np.int32).ptr,
                                                      put(col_k, np.int32).ptr, nk, edges_d.ptr, T, nbins, ncols,
                                                      work.ptr, out.ptr), "spyhip_psth_proportion")
            return out.numpy(), columns
        finally:
            self.synchronize()
            for b in bufs:
                b.free()

    # ---- operator arithmetic on data objects
    def arith(self, op, base, trials, operand=0.0, operand_trials=None, channels=None, dtype=None):
        """`trial (op) operand` for the trials of `base` (rows x ..., float32 / float64 / complex64 / complex128), stacked:
        `trials` (T, 2) are [start, stop) rows, `op` one of 'add', 'sub', 'mul', 'div', 'rsub', 'rdiv' (operand - trial,
        operand / trial), 'pow' and the one-argument 'square', 'copy', 'ones', 'sqrt'.  `operand`: a scalar, an array that
        broadcasts to every trial, or with `operand_trials` (T, 2) a second matrix whose trials pair up with the base's.
        `channels`: indices into the last axis of `base`; `dtype`: the result type (default: NumPy's for base and operand).
        See spyhip_arith in include/spyhip.h."""
        from .datatype.arithmetic import ARITH_OP, ARITH_TYPE, arith_view
        base = np.ascontiguousarray(base)
        trl = np.asarray(trials, dtype=np.int64).reshape(-1, 2)
        n = trl[:, 1] - trl[:, 0]
        if base.ndim < 1 or base.ndim > 4 or np.any(n < 0) or np.any(trl[:, 0] < 0) or np.any(trl[:, 1] > base.shape[0]):
            raise ValueError("base must have 1 to 4 dimensions and hold the rows of every trial")
        starts = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
        array = None if np.isscalar(operand) else np.asarray(operand)
        if dtype is None:
            dtype = np.result_type(base.dtype, operand if array is None else array.dtype)
        dtype = np.dtype(dtype)
        chan = None if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        inner = base.shape[1:] if chan is None else base.shape[1:-1] + (chan.size,)
        brow, mode, scalar, extent, stride, b_rows = starts[:-1], 0, 0.0, None, None, 0
        bufs = []
        try:
            if array is None:
                scalar = operand
            elif operand_trials is None:
                array = np.ascontiguousarray(array, dtype=dtype)
                extent, stride = arith_view(array.shape, inner)
                mode, b_rows = 1, array.size
            else:
                array = np.ascontiguousarray(array, dtype=dtype)
                otrl = np.asarray(operand_trials, dtype=np.int64).reshape(-1, 2)
                if array.shape[1:] != inner or not np.array_equal(otrl[:, 1] - otrl[:, 0], n):
                    raise ValueError("the operand's trials must have the shapes of the base's")
                brow, mode, b_rows = otrl[:, 0], 2, array.shape[0]
            desc = np.ascontiguousarray(np.stack([starts[:-1], trl[:, 0], brow, n], axis=1))
            a_d = self._put(base, base.dtype)
            bufs.append(a_d)
            out = Buffer(self, (int(starts[-1]),) + tuple(inner), dtype)
            bufs.append(out)
            if out.nbytes == 0:
                return np.empty(out.shape, dtype=dtype)
            b_d = None
            if array is not None:
                b_d = self._put(array, dtype)
                bufs.append(b_d)
            desc_d, chan_d = self._put(desc, np.int64), None if chan is None else self._put(chan, np.int32)
            bufs += [desc_d] + ([] if chan_d is None else [chan_d])
            i64p = lambda x: None if x is None else x.ctypes.data_as(_lib.c_i64p)      # noqa: E731
            check(self.lib.spyhip_arith(self.handle, ARITH_OP[op], mode, ARITH_TYPE[base.dtype], ARITH_TYPE[dtype], a_d.ptr,
                                        base.shape[0], None if b_d is None else b_d.ptr, b_rows, i64p(extent), i64p(stride),
                                        float(np.real(scalar)), float(np.imag(scalar)), i64p(desc), desc_d.ptr,
                                        desc.shape[0], int(np.prod(inner, dtype=np.int64)),
                                        None if chan is None else chan.ctypes.data_as(_lib.c_i32p),
                                        None if chan_d is None else chan_d.ptr, int(inner[-1]) if inner else 1,
                                        int(base.shape[-1]), out.ptr, out.shape[0]), "spyhip_arith")
            return out.numpy()
        finally:
            self.synchronize()
            for b in bufs:
                b.free()

    # ---- data selection
    def select(self, data, trials, axes=None):
        """The trials of `data` (rows x up to three inner axes; elements of 4, 8 or 16 bytes), stacked: `trials` (T, 2)
        are [start, stop) rows, in any order, repeated or empty; `axes`: per inner axis None (all of it), (start, count)
        or an array of indices.  What `np.concatenate([data[a:b][np.ix_(...)] ...])` gives, bit for bit.  See
        spyhip_select in include/spyhip.h."""
        from .datatype.selectdata import select_axes
        data = np.ascontiguousarray(data)
        trl = np.asarray(trials, dtype=np.int64).reshape(-1, 2)
        n = trl[:, 1] - trl[:, 0]
        if data.ndim < 1 or data.ndim > 4 or np.any(n < 0) or np.any(trl[:, 0] < 0) or np.any(trl[:, 1] > data.shape[0]):
            raise ValueError("data must have 1 to 4 dimensions and hold the rows of every trial")
        extent, kind, start, count, idx = select_axes(data.shape[1:], axes)
        starts = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
        desc = np.ascontiguousarray(np.stack([starts[:-1], trl[:, 0], n], axis=1))
        shape = (int(starts[-1]),) + tuple(int(c) for c in count[4 - data.ndim:])
        if int(np.prod(shape)) == 0:
            return np.empty(shape, dtype=data.dtype)
        bufs = []
        try:
            src_d, out = self._put(data, data.dtype), Buffer(self, shape, data.dtype)
            bufs += [src_d, out]
            desc_d, idx_d = self._put(desc, np.int64), None if idx is None else self._put(idx, np.int32)
            bufs += [desc_d] + ([] if idx_d is None else [idx_d])
            check(self.lib.spyhip_select(self.handle, data.dtype.itemsize, src_d.ptr, data.shape[0],
                                         extent.ctypes.data_as(_lib.c_i64p), kind.ctypes.data_as(_lib.c_i32p),
                                         start.ctypes.data_as(_lib.c_i64p), count.ctypes.data_as(_lib.c_i64p),
                                         None if idx is None else idx.ctypes.data_as(_lib.c_i32p),
                                         None if idx_d is None else idx_d.ptr, desc.ctypes.data_as(_lib.c_i64p), desc_d.ptr,
                                         desc.shape[0], out.ptr, shape[0]), "spyhip_select")
            return out.numpy()
        finally:
            self.synchronize()
            for b in bufs:
                b.free()

    # ---- channel concatenation
    def concat(self, sources, trials=None, pre=1):
        """The trials of 2 .. 8 arrays side by side, stacked: `sources` are arrays of one dtype (elements of 4, 8 or 16
        bytes) whose first axis are the rows and whose rows are `pre` lines; `trials` (nsources, T, 2) are the [start, stop)
        rows of trial t in each source (the same length in all of them; default: every source whole, one trial).  In every
        line of the result the line of source s follows that of source s - 1: with pre = 1 what
        `np.concatenate([np.concatenate([x[a:b].reshape(b - a, -1) ...], axis=1) ...])` gives, bit for bit, as a matrix
        of rows.  See spyhip_concat in include/spyhip.h."""
        sources = [np.ascontiguousarray(x) for x in sources]
        nsrc, pre = len(sources), int(pre)
        if nsrc < 2 or any(x.ndim < 1 or x.dtype != sources[0].dtype for x in sources) or pre < 1:
            raise ValueError("sources must be two or more arrays of one dtype")
        dtype = sources[0].dtype
        if trials is None:
            trials = [[[0, x.shape[0]]] for x in sources]
        trl = np.asarray(trials, dtype=np.int64).reshape(nsrc, -1, 2)
        n = trl[0, :, 1] - trl[0, :, 0]
        if np.any(n < 0) or np.any(trl[:, :, 1] - trl[:, :, 0] != n) or np.any(trl[:, :, 0] < 0) or \
                any(np.any(trl[s, :, 1] > x.shape[0]) for s, x in enumerate(sources)):
            raise ValueError("every source must hold the rows of every trial, and a trial has the same rows in all of them")
        width = [int(np.prod(x.shape[1:], dtype=np.int64)) for x in sources]
        if any(w % pre or w == 0 for w in width):
            raise ValueError("every source's rows must be `pre` lines")
        starts = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
        desc = np.ascontiguousarray(np.concatenate([starts[:-1, None], n[:, None], trl[:, :, 0].T], axis=1))
        shape = (int(starts[-1]), sum(width))
        if shape[0] == 0:
            return np.empty(shape, dtype=dtype)
        run = np.array([w // pre for w in width], dtype=np.int64)
        rows = np.array([x.shape[0] for x in sources], dtype=np.int64)
        bufs = []
        try:
            for x in sources:
                bufs.append(self._put(x, dtype))
            ptrs = (C.c_void_p * nsrc)(*[b.ptr.value for b in bufs])
            out, desc_d = Buffer(self, shape, dtype), self._put(desc, np.int64)
            bufs += [out, desc_d]
            check(self.lib.spyhip_concat(self.handle, dtype.itemsize, nsrc, ptrs, rows.ctypes.data_as(_lib.c_i64p),
                                         run.ctypes.data_as(_lib.c_i64p), pre, desc.ctypes.data_as(_lib.c_i64p), desc_d.ptr,
                                         desc.shape[0], out.ptr, shape[0]), "spyhip_concat")
            return out.numpy()
        finally:
            self.synchronize()
            for b in bufs:
                b.free()

    # ---- synthetic data: the deterministic part of a trial, from noise the host drew
    def _synth(self, bufs, out, call, name):
        try:
            check(call(out.ptr), name)
            return out.numpy()
        finally:
            self.synchronize()
            for b in bufs + [out]:
                b.free()

    def synth_ar2(self, noise, AdjMat, alphas=(0.55, -0.8)):
        """The AR(2) network of synthdata.ar2_network driven by `noise` ((ntrials, nsamples, nchan) float64 innovations
        whose first two samples are the initial values): (ntrials, nsamples, nchan) float32.  See spyhip_synth_ar2 in
        include/spyhip.h."""
        from .synthdata import coupling_table
        noise = np.ascontiguousarray(noise, dtype=np.float64)
        if noise.ndim != 3:
            raise ValueError("noise must be (ntrials, nsamples, nchan)")
        rowptr, col, w = coupling_table(AdjMat)
        if rowptr.size != noise.shape[2] + 1:
            raise ValueError("AdjMat must be (nchan, nchan)")
        if noise.shape[0] == 0:
            return np.empty(noise.shape, dtype=np.float32)
        bufs = [self._put(noise, np.float64), self._put(rowptr, np.int32)]
        if col.size:
            bufs += [self._put(col, np.int32), self._put(w, np.float32)]
        col_d, w_d = (bufs[2].ptr, bufs[3].ptr) if col.size else (None, None)
        T, n, c = noise.shape
        return self._synth(bufs, Buffer(self, noise.shape, np.float32), lambda out: self.lib.spyhip_synth_ar2(
            self.handle, bufs[0].ptr, T, n, c, float(alphas[0]), float(alphas[1]), rowptr.ctypes.data_as(_lib.c_i32p),
            col.ctypes.data_as(_lib.c_i32p), bufs[1].ptr, col_d, w_d, out), "spyhip_synth_ar2")

    def synth_phase(self, wn, lin, ps0, rel_eps, want_cos=True):
        """(lin[i] + ps0[t][c]) + cumsum((float)rel_eps * wn) along the samples, or its cosine, float32.  wn: (ntrials,
        nsamples, nchan); lin: (nsamples); ps0: (ntrials, nchan).  See spyhip_synth_phase in include/spyhip.h."""
        wn = np.ascontiguousarray(wn, dtype=np.float32)
        if wn.ndim != 3:
            raise ValueError("wn must be (ntrials, nsamples, nchan)")
        T, n, c = wn.shape
        lin, ps0 = np.ascontiguousarray(lin, dtype=np.float32), np.ascontiguousarray(ps0, dtype=np.float32)
        if lin.shape != (n,) or ps0.shape != (T, c):
            raise ValueError("lin must be (nsamples) and ps0 (ntrials, nchan)")
        if wn.size == 0:
            return np.empty(wn.shape, dtype=np.float32)
        bufs = [self._put(wn, np.float32), self._put(lin, np.float32), self._put(ps0, np.float32)]
        return self._synth(bufs, Buffer(self, wn.shape, np.float32), lambda out: self.lib.spyhip_synth_phase(
            self.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, float(rel_eps), T, n, c, int(bool(want_cos)), out),
            "spyhip_synth_phase")

    def synth_tile(self, col, ntrials, nchan):
        """out[t][i][c] = col[i]: (ntrials, len(col), nchan) float32.  See spyhip_synth_tile in include/spyhip.h."""
        col = np.ascontiguousarray(col, dtype=np.float32).reshape(-1)
        shape = (int(ntrials), col.size, int(nchan))
        if int(np.prod(shape)) == 0:
            return np.empty(shape, dtype=np.float32)
        bufs = [self._put(col, np.float32)]
        return self._synth(bufs, Buffer(self, shape, np.float32), lambda out: self.lib.spyhip_synth_tile(
            self.handle, bufs[0].ptr, shape[0], shape[1], shape[2], out), "spyhip_synth_tile")

    def close(self):
        if self.handle is not None:
            self.lib.spyhip_ctx_destroy(self.handle)
        self.handle = None
