#!/usr/bin/env python3
"""GPU timing of the tolerant seeded stage A (msspe_kmer_candidates_tolerant_packed_dev) at BASELINE configs[2]'s
shape: msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed form, segment 500 / stride 250 / window 50,
k = 13, the 572-primer panel of tests/golden/config2_10k.json as seeds (its F primers in direction 0, its R primers in
direction 1).  Every call is event-timed on the device around the blocking call, best of --repeats after a warm-up.

Per direction, in one session on one context:
  plain / seeded / sets / tolerant_n0   the unseeded call, the exact-seeded call on the same seeds, the _sets call with
                                        one excluded word, the tolerant call without seeds
  tolerant M0 / M2E3 / END1 30          the tolerant call under three rules, with its own phases (msspe_get_info
                                        "stage_a_tolerant_incidence_us" / "_seed_us") and its winners beside the
                                        exact-seeded count
and once: msspe_segment_coverage_mm with counts (M = 2, E = 3) and msspe_panel_thin_thal's listing and scoring phases
on the whole panel -- the yardsticks of the incidence pass.

    python tools/perf_stage_a_tolerant.py [--rows 10000] [--length 30000] [--repeats 3] [--package DIR] [--baseline]

--package: import msspe_amd from another checkout's open-msspe-design_amd (a build of the parent commit);
--baseline: only the calls that exist there (plain, seeded, sets).  Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--package", default=str(ROOT / "open-msspe-design_amd"))
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import torch
    import msspe_amd as m

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    panel = [fx["primers_kept"]["F"], fx["primers_kept"]["R"]]
    rows, length = args.rows, args.length
    g = m.synth.aligned_genomes(rows, length)
    mm = max(1, min(10, -(-rows // 50)))
    opt = m.KmerOpt(500, 250, 50, 13, 1000, mm)
    eng = m.Engine(0)
    d = eng.put_rows_packed(g)

    def timed(call):
        best, out = None, None
        for rep in range(args.repeats + 1):   # the first call is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if rep and (best is None or ms < best[0]):
                best = (ms, out, {key: eng.info(key) for key in info_keys})
        return best

    info_keys: list[str] = []
    try:
        for direction in (0, 1):
            seed = panel[direction]
            ms, (w, f), _ = timed(lambda: eng.kmer_candidates_packed(d, rows, length, opt, direction))
            line = {"direction": direction, "seeds": len(seed), "plain_ms": round(ms, 3), "plain_winners": len(w)}
            ms, (ws, _), _ = timed(lambda: eng.kmer_candidates_packed(d, rows, length, opt, direction, seed=seed))
            line.update(seeded_ms=round(ms, 3), seeded_winners=len(ws))
            ms, (wx, _), _ = timed(lambda: eng.kmer_candidates_packed(d, rows, length, opt, direction, seed=seed,
                                                                       exclude=[w[-1]]))
            line.update(sets_ms=round(ms, 3), sets_winners=len(wx))
            if not args.baseline:
                ms, out, _ = timed(lambda: eng.kmer_candidates_tolerant_packed(d, rows, length, opt, direction, [],
                                                                               m.seed_rule(2, 3)))
                assert out[0] == w
                line.update(tolerant_n0_ms=round(ms, 3))
            print(json.dumps(line), flush=True)
            if args.baseline:
                continue
            info_keys[:] = ["stage_a_tolerant_" + key for key in ("tiles", "segments", "incidence_us", "seed_us")]
            chem = m.Chem.ntthal()
            for label, rule in (("M0", m.seed_rule(0, 3)), ("M2E3", m.seed_rule(2, 3)),
                                ("END1_30", m.seed_rule(2, 3, "end1", chem, 30.0))):
                ms, out, info = timed(lambda: eng.kmer_candidates_tolerant_packed(d, rows, length, opt, direction, seed,
                                                                                  rule))
                if label == "M0":
                    assert out[0] == ws, "mode 0 without mismatches is the exact-seeded call"
                print(json.dumps({"direction": direction, "rule": label, "call_ms": round(ms, 3),
                                  "winners": len(out[0]), "exact_seeded_winners": len(ws), "covered": int(out[2].sum()),
                                  "segments": int(out[2].size), "tiles": info[info_keys[0]],
                                  "incidence_ms": info[info_keys[2]] / 1e3, "seed_ms": info[info_keys[3]] / 1e3}),
                      flush=True)
            info_keys[:] = []
        if not args.baseline:
            copt = m.KmerOpt(500, 250, 50, 13, 0, 0)
            ms, _, _ = timed(lambda: eng.segment_coverage_mm_packed(d, rows, length, copt, panel[0], panel[1], 2, 3,
                                                                    per_primer=True))
            print(json.dumps({"case": "coverage_mm_with_counts", "M": 2, "E": 3, "call_ms": round(ms, 3)}), flush=True)
            info_keys[:] = ["panel_thin_thal_" + key for key in ("list_us", "unique_us", "score_us", "fold_us")]
            ms, _, info = timed(lambda: eng.panel_thin_thal((d, rows, length), copt, panel[0], panel[1], 2, 3,
                                                            m.Chem.ntthal(), "end1", 30.0, form="packed"))
            print(json.dumps({"case": "panel_thin_thal", "call_ms": round(ms, 3),
                              **{key[len("panel_thin_thal_"):-3] + "_ms": v / 1e3 for key, v in info.items()}}), flush=True)
    finally:
        eng.device_free(d)
        eng.close()


if __name__ == "__main__":
    main()
