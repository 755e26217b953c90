"""Sessions of randomised calls over the newer entry points on ONE long-lived context (tests/session_campaign_model.py,
the campaign of tools/random_campaign_session.py): one engine per committed seed, a schedule that grows and shrinks
every family, runs the families that share work areas of the context straight after each other, pre-fills every device
output with a sentinel and sets engine options between calls.  Every call is compared exactly with the CPU oracle or the
family's numpy model, everything behind an output's defined extent has to stay the sentinel, and the first three calls,
repeated at the end of the session, have to return the same bytes."""
import pytest

import session_campaign_model as scm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", scm.SEEDS)
def test_session(seed):
    import msspe_amd
    eng = msspe_amd.Engine(0)
    try:
        failures = scm.run_session(seed, eng, msspe_amd)
    finally:
        eng.close()
    assert not failures, "\n".join(failures)
