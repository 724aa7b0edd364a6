"""pytest plugin (`PYTHONPATH=tools python -m pytest -p pytest_intervals ...`): the interval of every test on three
clocks (monotonic, boottime, realtime; ns), written as JSON to $TEST_INTERVALS_OUT (test_intervals.json) so that a
kernel trace of the run can be split by test (tools/kernel_map.py)."""
import json
import os
import time

import pytest

_rec = []


def _now():
    return time.clock_gettime_ns(time.CLOCK_MONOTONIC), time.clock_gettime_ns(time.CLOCK_BOOTTIME), time.time_ns()


@pytest.hookimpl(hookwrapper=True)
def pytest_runtest_protocol(item, nextitem):
    t0 = _now()
    yield
    _rec.append({"id": item.nodeid, "t0": t0, "t1": _now()})


def pytest_sessionfinish(session, exitstatus):
    out = os.environ.get("TEST_INTERVALS_OUT", "test_intervals.json")
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(_rec, f)
