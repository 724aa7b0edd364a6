"""SpikeData: the spike table spy.spike_psth reads (syncopy/datatype/discrete_data.py: DiscreteData, SpikeData), in
memory and - as three columns - in HBM.

`data` is an (nSpikes, 3) int64 array with the columns ["sample", "channel", "unit"]; a trial owns the rows whose sample
lies in [start, end) of its trial definition, spikes between trials belong to none (`trialid` -1).

Deviations from the reference, on purpose:
  * the rows are sorted stably by sample at construction when they are not already.  The reference finds a trial's rows
    with np.searchsorted(samples, sampleinfo.ravel()) (discrete_data.py:186-196) and never sorts, so unsorted input gives
    it arbitrary trials; the kernels rely on the order;
  * channels and units are non-negative and below 2^31 (they travel as int32), any integer dtype or floats that hold
    integers are accepted, and the table is held as int64;
  * `.spike` containers are neither saved nor loaded, and there are no waveforms.
"""
import numpy as np

from . import _Base
from ..shared.errors import SPYTypeError, SPYValueError

__all__ = ["SpikeData", "SpikeSelection"]


class SpikeData(_Base):
    _defaultDimord = ["sample", "channel", "unit"]

    def __init__(self, data=None, samplerate=None, trialdefinition=None, dimord=None, channel=None, unit=None):
        if dimord is not None and sorted(dimord) != sorted(self._defaultDimord):
            raise SPYValueError(f"a permutation of {self._defaultDimord}", varname="dimord", actual=str(list(dimord)))
        self._rows = None
        self._trialid = None
        self._trialdefinition = None
        self.channel_idx = self.unit_idx = None
        self.channel = self.unit = None
        super().__init__(data, samplerate, None, dimord)
        if self._data is not None:
            self.trialdefinition = trialdefinition
            if channel is not None:
                self.channel = self._labels(channel, self.channel_idx, "channel")
            if unit is not None:
                self.unit = self._labels(unit, self.unit_idx, "unit")
        elif trialdefinition is not None:
            raise SPYValueError("non-empty SpikeData", varname="trialdefinition", actual="a trial definition without data")

    @staticmethod
    def _labels(labels, idx, what):
        labels = np.array(labels)
        if labels.ndim != 1 or labels.size != idx.size:
            raise SPYValueError(f"exactly {idx.size} {what} label(s)", varname=what, actual=str(labels.shape))
        return labels

    # ---- the table
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, value):
        if value is None:
            self._data = None
            self._rows = self._trialid = None
            self.invalidate()
            return
        arr = np.asarray(value)
        if arr.dtype.kind not in "iuf":
            raise SPYTypeError(arr.dtype, varname="data", expected="integer like")
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise SPYValueError("(nSpikes, 3) array", varname="data", actual=f"shape {arr.shape}")
        if arr.shape[0] == 0:
            raise SPYValueError("non empty data set", varname="data")
        if arr.dtype.kind == "f":
            if not np.all(np.isfinite(arr)) or np.any(arr != np.rint(arr)) or np.any(np.abs(arr) >= 2.0 ** 63):
                raise SPYTypeError(arr.dtype, varname="data", expected="integer like")
        elif arr.dtype == np.uint64 and arr.max() >= 2 ** 63:
            raise SPYValueError("values below 2^63", varname="data", actual=str(arr.max()))
        arr = arr.astype(np.int64)[:, [self.dimord.index(name) for name in self._defaultDimord]]
        self.dimord = list(self._defaultDimord)
        for col, name in ((1, "channel"), (2, "unit")):
            lo, hi = int(arr[:, col].min()), int(arr[:, col].max())
            if lo < 0 or hi >= 2 ** 31:
                raise SPYValueError(f"{name} numbers in [0, 2^31)", varname="data", actual=f"{lo} ... {hi}")
        if np.any(np.diff(arr[:, 0]) < 0):
            arr = arr[np.argsort(arr[:, 0], kind="stable")]
        self._data = np.ascontiguousarray(arr)
        self._pending = None
        self.invalidate()
        self.channel_idx = np.unique(arr[:, 1])
        self.unit_idx = np.unique(arr[:, 2])
        if self.channel is None or len(self.channel) != self.channel_idx.size:
            self.channel = self._default_channel_labels()
        if self.unit is None or len(self.unit) != self.unit_idx.size:
            self.unit = self._default_unit_labels()
        if self._trialdefinition is not None:
            self._assign_trials()

    def _default_channel_labels(self):
        chan_max = self.channel_idx.max()
        return np.array(["channel" + str(int(i + 1)).zfill(len(str(chan_max))) for i in self.channel_idx])

    def _default_unit_labels(self):
        unit_max = self.unit_idx.max()
        return np.array(["unit" + str(int(i + 1)).zfill(len(str(unit_max))) for i in self.unit_idx])

    @property
    def sample(self):
        return None if self._data is None else self._data[:, 0]

    # ---- trials
    @property
    def trialdefinition(self):
        return self._trialdefinition

    @trialdefinition.setter
    def trialdefinition(self, trl):
        if self._data is None:
            raise SPYValueError("non-empty SpikeData", varname="trialdefinition", actual="a trial definition without data")
        if trl is None:                                   # one trial from the first to the last spike, as the reference
            trl = [[self._data[0, 0], self._data[-1, 0], 0]]
        _Base.trialdefinition.fset(self, trl)
        if np.any(self._trialdefinition[:, :2] < 0) or not np.all(np.isfinite(self._trialdefinition)):
            self._trialdefinition = None
            raise SPYValueError("finite, non-negative sample numbers", varname="trialdefinition")
        self._assign_trials()

    def _assign_trials(self):
        si = self.sampleinfo
        self._rows = np.searchsorted(self._data[:, 0], si.ravel()).reshape(si.shape).astype(np.int64)
        self._rows[:, 1] = np.maximum(self._rows[:, 1], self._rows[:, 0])
        trialid = np.full(self._data.shape[0], -1, dtype=int)
        for k, (a, b) in enumerate(self._rows):
            trialid[a:b] = k
        self._trialid = trialid

    @property
    def trial_rows(self):
        """(nTrials, 2) int64: the rows [first, last + 1) of the table that every trial owns"""
        return self._rows

    @property
    def trialid(self):
        """trial of every spike, -1 for spikes between trials"""
        return self._trialid

    @property
    def trials(self):
        return [self._data[a:b] for a, b in self._rows]

    @property
    def time(self):
        """trigger-relative time of every spike, trial by trial: (sample - start + offset) / samplerate"""
        return [(self._data[a:b, 0] - self.sampleinfo[k, 0] + self._trialdefinition[k, 2]) / self.samplerate
                for k, (a, b) in enumerate(self._rows)]

    def selectdata(self, select=None):
        self.selection = None if select is None else SpikeSelection(self, select)
        return self

    # ---- the device copy
    def device_columns(self, device=None):
        """(sample int64, channel int32, unit int32): the table as three contiguous arrays in HBM, 16 bytes per spike,
        uploaded once and kept until `.data` is assigned or invalidate() is called"""
        import torch
        from .. import backend
        backend.require_gpu()
        dev = torch.device("cuda" if device is None else device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (id(self._data), self._data.shape, str(dev))
        if self._device is None or self._device_key != key:
            cols = (np.ascontiguousarray(self._data[:, 0]), self._data[:, 1].astype(np.int32),
                    self._data[:, 2].astype(np.int32))
            self._device = tuple(torch.from_numpy(c).to(dev) for c in cols)
            self._device_key = key
        return self._device


class SpikeSelection:
    """Resolved in-place selection of SpikeData.

    trials : any order, repeats allowed, kept as given
    channel, unit : indices into `data.channel` / `data.unit` (the labels of the distinct channel and unit numbers, in
             ascending order), labels, or a slice; held as the NUMBERS that stand in the table
    The time window of spy.spike_psth is its `latency` argument: a "latency" key is refused here."""

    def __init__(self, data, select):
        if not isinstance(select, dict):
            raise SPYTypeError(select, "select", "dict")
        if "latency" in select:
            raise SPYValueError("keys 'trials', 'channel', 'unit'; the time window is the `latency=` argument of "
                                "spy.spike_psth", varname="select", actual="latency")
        unknown = set(select) - {"trials", "channel", "unit"}
        if unknown:
            raise SPYValueError("keys 'trials', 'channel', 'unit'", varname="select", actual=str(sorted(unknown)))
        self.select = dict(select)
        ntr = data.trialdefinition.shape[0]
        tr = select.get("trials")
        if tr is None or (isinstance(tr, str) and tr == "all"):
            self.trial_ids = list(range(ntr))
        else:
            self.trial_ids = [int(t) for t in np.atleast_1d(tr)]
            if any(t < 0 or t >= ntr for t in self.trial_ids):
                raise SPYValueError(f"trial indices in [0, {ntr})", varname="select: trials", actual=str(tr))
        self.channel = self._numbers(select.get("channel"), list(data.channel), data.channel_idx, "channel")
        self.unit = self._numbers(select.get("unit"), list(data.unit), data.unit_idx, "unit")
        self.trialdefinition = data.trialdefinition[self.trial_ids, :]
        self._samplerate = data.samplerate

    @staticmethod
    def _numbers(spec, names, numbers, what):
        if spec is None or (isinstance(spec, str) and spec == "all"):
            return [int(n) for n in numbers]
        if isinstance(spec, slice):
            return [int(n) for n in numbers[spec]]
        idx = []
        for s in np.atleast_1d(spec):
            if isinstance(s, (str, np.str_)):
                if s not in names:
                    raise SPYValueError(f"existing {what} names", varname=f"select: {what}", actual=str(s))
                idx.append(names.index(s))
            else:
                idx.append(int(s))
        if any(i < 0 or i >= len(names) for i in idx):
            raise SPYValueError(f"{what} indices in [0, {len(names)})", varname=f"select: {what}", actual=str(spec))
        return [int(numbers[i]) for i in idx]

    @property
    def sampleinfo(self):
        return self.trialdefinition[:, :2].astype(np.int64)

    @property
    def trialintervals(self):
        si, off = self.sampleinfo, self.trialdefinition[:, 2]
        n = si[:, 1] - si[:, 0]
        return np.stack([off, off + n - 1], axis=1) / self._samplerate
