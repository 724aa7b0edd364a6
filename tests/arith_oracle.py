"""The oracle of the operator arithmetic: NumPy itself, applied per selected trial as the reference's arithmetic_cF does
(datatype/methods/arithmetic.py:416-470), the trials restacked in selection order and stored in the result type."""
import numpy as np

from syncopy_amd.statistics.summary_stats import _selected_trials

OPS = {"+": lambda x, y: x + y, "-": lambda x, y: x - y, "*": lambda x, y: x * y, "/": lambda x, y: x / y,
       "**": lambda x, y: x ** y}


def arith(base, operand, operator, reflected=False):
    """the stacked result of `base (operator) operand` (`operand (operator) base` if reflected); operand: a scalar, an
    array, or a data object, whose trials pair up with the base's"""
    trials = [x for x, _ in _selected_trials(base)]
    if hasattr(operand, "trialdefinition"):
        others = [y for y, _ in _selected_trials(operand)]
        opres = np.result_type(*(x.dtype for x in trials), *(y.dtype for y in others))
    else:
        others = [operand if np.isscalar(operand) else np.array(operand)] * len(trials)
        opres = np.result_type(*(x.dtype for x in trials), operand if np.isscalar(operand) else others[0].dtype)
    with np.errstate(all="ignore"):
        res = [OPS[operator](y, x) if reflected else OPS[operator](x, y) for x, y in zip(trials, others)]
    return np.concatenate(res, axis=0).astype(opres)
