"""Fixture generator for the egress test of the `.spy` container (tests/test_spy_container.py): this package's `spy.save`
writes the reference-written recording, power spectrum and cross-spectral density of tests/golden/spy_container/session.spy
into a new container.  Each object's log (times, user, host and paths of the run that wrote the source) is replaced by
a fixed text and no new entries are added, so that the files depend on nothing but the inputs.
`oracle/make_golden.sh --egress` runs it into tests/golden/spy_container/egress.spy and then loads that container with the
unmodified reference (`--check-container`).  TEST INFRASTRUCTURE ONLY."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "..", "tests", "golden", "spy_container", "session.spy")


def write_egress(cont):
    """Save the three objects into the container `cont` (its name is stored in the files: keep it `egress.spy`)."""
    import syncopy_amd as spy
    from syncopy_amd.io import spy_container
    entry = spy_container._log_entry
    spy_container._log_entry = lambda text: ""
    try:
        src = spy.load(SOURCE)
        for obj in src.values():
            obj.log = "\n\n|=== egress fixture ===|\n\n\tloaded from session.spy"
        spy.save(src["session.analog"], container=cont)
        spy.save(src["session_pow.spectral"], container=cont, tag="pow")
        spy.save(src["session_csd.crossspectral"], container=cont, tag="csd")
    finally:
        spy_container._log_entry = entry


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(HERE, ".."))
    write_egress(sys.argv[1])
