"""Device time of the panel thinning (msspe_panel_thin_packed_dev) at config2 size: msspe_amd.synth.aligned_genomes(10000,
30000) resident in packed form, segment 500 / stride 250 / window 50, k 13, up to 2 mismatches, last 3 bases exact,
min_gain 1, for two primer sets of tests/golden/config2_10k.json: the 572 kept primers, and the unfiltered stage-A
winners of both directions (1,225).  In the same session, on the same inputs, msspe_segment_coverage_mm_packed_dev
with per-primer counts: the incidence pass does the same comparisons and stores words instead of adding popcounts.

    python tools/perf_panel_thin.py [--rows 10000] [--length 30000] [--reps 3]

The phases are the call's own device times between events on its stream (msspe_get_info "panel_thin_incidence_us",
"panel_thin_gain0_us", "panel_thin_rounds_us"), the best of --reps calls after one warm-up; the with-counts figure is
device time between two events around the call (it copies best and the counts back), the best of --reps likewise.
Prints one JSON line per primer set."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    sets = [("kept", fx["primers_kept"]["F"], fx["primers_kept"]["R"]),
            ("stage_a_winners", [w for w, _ in fx["winners"]["0"]], [w for w, _ in fx["winners"]["1"]])]
    g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
    n, L = g.shape
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    hp = eng.put_rows_packed(g)
    opt = msspe_amd.KmerOpt(500, 250, 50, 13, 0, 0)
    M, E = 2, 3
    try:
        for name, fwd, rev in sets:
            f, r = msspe_amd.pack_oligos(fwd), msspe_amd.pack_oligos(rev)
            best = None
            for rep in range(args.reps + 1):
                keep, order, gains, covered, c_all, c_kept = eng.panel_thin((hp, n, L), opt, f, r, M, E, form="packed")
                us = [eng.info("panel_thin_%s_us" % ph) for ph in ("incidence", "gain0", "rounds")]
                if rep and (best is None or sum(us) < sum(best)):
                    best = us
            rounds, groups = eng.info("panel_thin_rounds"), eng.info("panel_thin_groups")
            counts_ms = None
            for rep in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, counts = eng.segment_coverage_mm_packed(hp, n, L, opt, f, r, M, E, per_primer=True)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    counts_ms = min(counts_ms or 1e30, e0.elapsed_time(e1))
            assert int(counts.sum()) >= c_all == c_kept
            print(json.dumps({"set": name, "n": len(f) + len(r), "kept": int(keep.sum()), "segments": int(covered.size),
                              "covered_all": c_all, "covered_kept": c_kept, "groups": groups,
                              "matrix_mb": round(groups * ((len(f) + len(r) + 63) // 64 * 64) * 8 / 2 ** 20, 1),
                              "incidence_ms": best[0] / 1e3, "gain0_ms": best[1] / 1e3, "rounds_ms": best[2] / 1e3,
                              "rounds": rounds, "us_per_round": round(best[2] / max(rounds, 1), 1),
                              "coverage_mm_with_counts_ms": round(counts_ms, 3),
                              "first_gains": gains[:5].tolist()}), flush=True)
    finally:
        eng.device_free(hp)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
