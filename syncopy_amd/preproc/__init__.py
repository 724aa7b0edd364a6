"""Time-domain preprocessing: `spy.preprocessing` (front end) and the host-side filter design."""
from .preprocessing import preprocessing  # noqa: F401
