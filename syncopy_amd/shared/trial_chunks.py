"""What the AnalogData front ends that work along time (spy.preprocessing, spy.resampledata, spy.timelockanalysis) share
between their argument checks and their kernels: the input checks, the in-place selection, and the way the selected
trials reach the device and the results their place in the stacked output.

`TrialSource.gather` hands out trials of one length as an (m, n, nchan) float32 device tensor by one of three routes:
  * a zero-copy view of the resident matrix (`AnalogData.device_data()`), when all channels are taken and the trials
    follow each other there;
  * a gather on the device (stack, and index_select for a channel subset) from the resident matrix otherwise;
  * a trial-by-trial upload from the host matrix when nothing is resident, or an upload is still in flight.
`equal_length_chunks` groups the trials by length and cuts the groups into chunks of a byte budget, and `ResultRows`
writes a chunk's result straight into the stacked result when its trials follow each other there, else block by block.
Nothing here needs a GPU by itself: the device is the resident tensor's, the caller's, or the current CUDA device.
"""
import contextlib
import functools

import numpy as np

from ..datatype import AnalogData, device_rows, require_real_analog, selected_channels
from .errors import SPYTypeError, SPYValueError


def check_analog_input(data):
    if not isinstance(data, AnalogData):
        raise SPYTypeError(data, varname="data", expected="Syncopy AnalogData object")
    if (data._data is None and data._pending is None) or data.trialdefinition is None:
        raise SPYValueError("non-empty Syncopy data object", varname="data", actual="empty object")
    require_real_analog(data)
    if data.dimord.index("time") != 0:
        raise SPYValueError("time x channel data", varname="data", actual=f"dimord {data.dimord}")


def reject_unknown_kwargs(kwargs, names):
    """`chan_per_worker` / `parallel` are accepted and ignored; `names` are the keywords the front end does take"""
    unknown = set(kwargs) - {"chan_per_worker", "parallel"}
    if unknown:
        raise SPYValueError(f"one of {sorted(names)}", varname="kwargs", actual=str(sorted(unknown)))


def check_scalar(v, varname, lims, int_like=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise SPYTypeError(v, varname=varname, expected="scalar")
    if not np.isfinite(v) and not (np.isinf(v) and np.isinf(lims[1]) and v > 0 and not int_like):
        raise SPYValueError(f"value to be greater or equals {lims[0]} and less or equals {lims[1]}", varname=varname,
                            actual=str(v))
    if int_like and float(v) != int(v):
        raise SPYValueError("integer-like value", varname=varname, actual=str(v))
    if v < lims[0] or v > lims[1]:
        raise SPYValueError(f"value to be greater or equals {lims[0]} and less or equals {lims[1]}", varname=varname,
                            actual=str(v))


@contextlib.contextmanager
def applied_selection(data, select):
    """`select` (if given) as the in-place selection of `data` inside the block, the selection it had before after it"""
    had_selection = data.selection
    try:
        if select is not None:
            data.selectdata(select)
        yield
    finally:
        data.selection = had_selection


def equal_length_chunks(lengths, nchan, chunk_bytes):
    """(n, ks): the trials `ks` of length n that go through a kernel together - trials of equal length, in the order the
    lengths first appear, at most `chunk_bytes` of float32 input (but at least one trial) at a time; empty trials are
    left out"""
    groups = {}
    for k, n in enumerate(lengths):
        groups.setdefault(int(n), []).append(k)
    for n, members in groups.items():
        if n < 1:
            continue
        per = max(1, chunk_bytes // (n * nchan * 4))
        for c0 in range(0, len(members), per):
            yield n, members[c0:c0 + per]


class TrialSource:
    """The selected trials `rows` (trial_rows(data)) and channels of `data`, from the resident matrix if there is one.
    The selection is read here, once: the object stays valid after the front end has restored the caller's."""

    def __init__(self, data, rows, device=None):
        self.data, self.rows, self._asked_device = data, rows, device
        self.chans = selected_channels(data)
        # a matrix that a copy thread is still filling is not read: those trials are uploaded on their own
        self.resident = data._device is not None and getattr(data, "_upload", None) is None
        self.src = data._device if self.resident else None
        self.src_rows = device_rows(data) if self.resident else rows
        nchan_in = int(data.data_shape[1])
        self.full = self.chans is None or list(self.chans) == list(range(nchan_in))
        self.nchan = nchan_in if self.full else len(self.chans)

    @functools.cached_property
    def dev(self):
        """the device the trials are handed out on (the host-only methods never ask for it)"""
        import torch
        if self._asked_device is not None:
            return torch.device(self._asked_device)
        return self.src.device if self.resident else torch.device("cuda", torch.cuda.current_device())

    @functools.cached_property
    def cidx(self):
        import torch
        return None if self.full else torch.as_tensor(list(self.chans), dtype=torch.int64, device=self.dev)

    def _host_block(self, a, b):
        blk = self.data.data[a:b]
        return blk if self.full else np.take(blk, self.chans, axis=1)

    def _device_block(self, a, b):
        blk = self.src[a:b]
        return blk if self.full else blk.index_select(1, self.cidx)

    def gather(self, ks, n):
        """(x, owned): the trials `ks`, all of length n, as an (m, n, nchan) float32 tensor on the device.  `owned` is
        False when x is a view of the resident matrix, which the caller must not write into."""
        import torch
        m, rows = len(ks), self.src_rows
        if self.resident and self.full and all(rows[ks[i + 1]][0] == rows[ks[i]][1] for i in range(m - 1)):
            return self.src[rows[ks[0]][0]:rows[ks[-1]][1]].view(m, n, self.nchan), False
        if self.resident:
            return torch.stack([self._device_block(*rows[k]) for k in ks]), True
        x = torch.empty((m, n, self.nchan), dtype=torch.float32, device=self.dev)
        for i, k in enumerate(ks):
            x[i].copy_(torch.from_numpy(np.ascontiguousarray(self._host_block(*rows[k]))))
        return x, True

    def host_trials(self):
        """the selected rows and channels of the host matrix, trial by trial"""
        return [self._host_block(a, b) for a, b in self.rows]

    def host_stack(self):
        """the same stacked in trial order (a view of the host matrix when they are one block of it)"""
        rows = self.rows
        if self.full and all(rows[i + 1][0] == rows[i][1] for i in range(len(rows) - 1)):
            return self.data.data[rows[0][0]:rows[-1][1]]
        return np.concatenate(self.host_trials(), axis=0)

    def fetch_rows(self):
        """host_stack() of an input that lives on the device only, from the resident matrix"""
        from .. import backend
        return np.concatenate([backend.to_host(self._device_block(a, b).contiguous()) for a, b in self.src_rows], axis=0)


class ResultRows:
    """The stacked (rows, nchan) result tensor `res` (of any dtype: the views and copies below are of its dtype), in which
    output trial k starts at row starts[k]."""

    def __init__(self, starts, res):
        self.starts, self.res = starts, res

    def view(self, ks, nout):
        """the (m, nout, nchan) view of the result that the trials `ks` of `nout` rows fill when they follow each other
        there, else None"""
        if any(ks[i + 1] != ks[i] + 1 for i in range(len(ks) - 1)):
            return None
        block = self.res[int(self.starts[ks[0]]):int(self.starts[ks[-1]] + nout)]
        return block.view(len(ks), nout, self.res.shape[1])

    def scatter(self, ks, nout, y):
        for i, k in enumerate(ks):
            self.res[int(self.starts[k]):int(self.starts[k] + nout)].copy_(y[i])
