"""The third session campaign on ONE long-lived context (tests/session_campaign3_model.py, the campaign of
tools/random_campaign_session.py --campaign 3): one engine per committed seed and a schedule of 27 calls -- thinning and
selection to a coverage depth, weighted thinning and selection, the conflict graph under both rules and the rule forms of
cover, tubes and select, the windowed bound first stage, the thal-scored passes through the one slab loop -- chained
with the older calls whose device state they share (ctx->thin, ctx->select, ctx->cover, ctx->graph, site_work, list U and
the packed tables), sizes alternating, every device output pre-filled with a sentinel, engine options set between
calls.  Every call is compared exactly with the CPU oracle or the family's numpy model, everything behind an output's
defined extent has to stay the sentinel, an all-ones weighted call equals the unweighted call run straight after it,
select_depth at R = 1 returns its neighbour select's bytes, the bound chain's last screen equals its first, and the
first three calls, repeated at the end of the session, have to return the same bytes."""
import pytest

import session_campaign3_model as s3

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", s3.SEEDS)
def test_session(seed):
    import msspe_amd
    eng = msspe_amd.Engine(0)
    try:
        failures = s3.run_session(seed, eng, msspe_amd)
    finally:
        eng.close()
    assert not failures, "\n".join(failures)
