"""NumPy model of spy.concat for the tests: `np.concatenate` of the sources' trials along the channel axis, stacked, with
the trial definition and the labels the result must carry.  Written from the reference's rules
(datatype/methods/concat.py), not from the front end's planner."""
import numpy as np


def join(sources, trials, axis):
    """trial k = rows [trials[s][k][0], trials[s][k][1]) of every source s, concatenated along `axis` (>= 1); the trials
    stacked along axis 0"""
    sources = [np.asarray(x) for x in sources]
    trials = np.asarray(trials, dtype=np.int64).reshape(len(sources), -1, 2)
    parts = [np.concatenate([x[a:b] for x, (a, b) in zip(sources, trials[:, k])], axis=axis) for k in range(trials.shape[1])]
    shape = list(sources[0].shape)
    shape[0], shape[axis] = 0, sum(x.shape[axis] for x in sources)
    return np.concatenate(parts, axis=0) if parts else np.empty(shape, dtype=sources[0].dtype)


def concat(objs):
    """(data, trialdefinition, channel labels or "default"): what spy.concat(*objs) must hold"""
    axis = objs[0].dimord.index("channel")
    data = join([o.data for o in objs], [o.trialdefinition[:, :2] for o in objs], axis)
    trl = np.array(objs[0].trialdefinition, dtype=float)
    n = trl[:, 1] - trl[:, 0]
    trl[:, 1] = np.cumsum(n)
    trl[:, 0] = trl[:, 1] - n
    names = [None if o.channel is None else [str(c) for c in o.channel] for o in objs]
    flat = [c for lab in names if lab is not None for c in lab]
    distinct = all(lab is not None for lab in names) and len(set(flat)) == len(flat)
    return data, trl, (flat if distinct else "default")
