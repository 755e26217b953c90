"""The second session campaign on ONE long-lived context (tests/session_campaign2_model.py, the campaign of
tools/random_campaign_session.py --campaign 2): one engine per committed seed and a schedule of 27 calls -- decision-only
screens through the bound chain, the bound diagnostic planes, coverage and thinning scored with thal, excluding and
tolerant stage A, the selection by coverage -- chained with the older calls whose device state they share (ctx->thin,
ctx->cover, site_work and the plane words, the chemistry cache), sizes alternating, every device output pre-filled with a
sentinel, engine options set between calls.  Every call is compared exactly with the CPU oracle or the family's numpy
model, everything behind an output's defined extent has to stay the sentinel, the bound chain's last screen equals its
first, and the first three calls, repeated at the end of the session, have to return the same bytes."""
import pytest

import session_campaign2_model as s2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", s2.SEEDS)
def test_session(seed):
    import msspe_amd
    eng = msspe_amd.Engine(0)
    try:
        failures = s2.run_session(seed, eng, msspe_amd)
    finally:
        eng.close()
    assert not failures, "\n".join(failures)
