#!/usr/bin/env python3
"""Randomised differential campaign over the newer entry points on ONE long-lived context (development aid, GPU): per
seed one Engine and a schedule of calls -- END, pool against pool, the thal record, seeded stage A, coverage within M
mismatches, panel thinning, cover and tubes, the background family -- in shuffled order, growing and shrinking, on dirty
output buffers and under engine options, each against the oracle or the family's model (tests/session_campaign_model.py),
and the first three calls once more at the end.  --campaign 2 drives the second campaign instead
(tests/session_campaign2_model.py): decision-only screens through the bound chain, the bound diagnostic planes, coverage
and thinning scored with thal, excluding and tolerant stage A and the selection by coverage, chained with the calls whose
device state they share.  --campaign 3 drives the third (tests/session_campaign3_model.py): thinning and selection to a
coverage depth, weighted coverage, the conflict graph under both rules with the rule forms of cover, tubes and select,
the windowed bound first stage and the one slab loop of the thal-scored passes, chained in the same way.
usage: random_campaign_session.py [seed] [sessions] [--campaign 1|2|3] [--models-only] [--only INDEX]
  --campaign N   1 (default): tests/session_campaign_model.py; 2: tests/session_campaign2_model.py;
                 3: tests/session_campaign3_model.py
  --models-only  no engine: every schedule and expected value, the model time per call and the counters per session
  --only INDEX   run the schedule up to and including call INDEX and check only that call"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "open-msspe-design_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))
args = sys.argv[1:]
models_only = "--models-only" in args
only = int(args[args.index("--only") + 1]) if "--only" in args else None
campaign = int(args[args.index("--campaign") + 1]) if "--campaign" in args else 1
if campaign not in (1, 2, 3):
    sys.exit("--campaign takes 1, 2 or 3")
if campaign == 3:
    import session_campaign3_model as scm
elif campaign == 2:
    import session_campaign2_model as scm
else:
    import session_campaign_model as scm
pos = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--only", "--campaign"))]
seed0 = int(pos[0]) if pos else 8
sessions = int(pos[1]) if len(pos) > 1 else 4
bad = 0
for seed in range(seed0, seed0 + sessions):
    if models_only:
        counts, seconds = scm.models_only(seed, log=lambda s: print(s, flush=True))
        print(f"session {seed}: model time {seconds:.1f} s, counters {counts}", flush=True)
        continue
    import msspe_amd as m
    t0 = time.perf_counter()
    eng = m.Engine(0)
    try:
        failures = scm.run_session(seed, eng, m, only=only, log=lambda s: print(s, flush=True))
    finally:
        eng.close()
    for f in failures:
        print("DIFFERS", f, flush=True)
    print(f"session {seed}: {len(failures)} failures, {time.perf_counter() - t0:.1f} s", flush=True)
    bad += len(failures)
print("BAD", bad)
sys.exit(1 if bad else 0)
