"""Time-domain preprocessing: `spy.preprocessing` and `spy.resampledata` (front ends) and the host-side filter design."""
from .preprocessing import preprocessing  # noqa: F401
from .resampledata import resampledata  # noqa: F401
