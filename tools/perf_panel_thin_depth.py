"""Device time of the panel thinning to a depth (msspe_panel_thin_depth_packed_dev) on the inputs of
tools/perf_panel_thin.py: msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed form, segment 500 / stride
250 / window 50, k 13, up to 2 mismatches, last 3 bases exact, min_gain 1, for the two primer sets of
tests/golden/config2_10k.json (the 572 kept primers; the 1,225 unfiltered stage-A winners), at R = 1, 2 and 3, beside
msspe_panel_thin_packed_dev from the same session.

    python tools/perf_panel_thin_depth.py [--rows 10000] [--length 30000] [--reps 3]

The phases are the call's own device times between events on its stream (msspe_get_info "panel_thin_incidence_us",
"panel_thin_depth_colsum_us", "panel_thin_gain0_us", "panel_thin_rounds_us"), the best total of --reps calls after one
warm-up.  Prints one JSON line per primer set and call; "vs_thin" is the call's device time over msspe_panel_thin's."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))

PHASES = ("incidence", "depth_colsum", "gain0", "rounds")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
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
            thin_ms = None
            for R in (0, 1, 2, 3):   # 0: msspe_panel_thin
                best = None
                for rep in range(args.reps + 1):
                    if R:
                        out = eng.panel_thin_depth((hp, n, L), opt, f, r, M, E, R, form="packed")
                    else:
                        out = eng.panel_thin((hp, n, L), opt, f, r, M, E, form="packed")
                    us = [eng.info("panel_thin_%s_us" % ph) if R or ph != "depth_colsum" else 0 for ph in PHASES]
                    if rep and (best is None or sum(us) < sum(best)):
                        best = us
                rounds = eng.info("panel_thin_rounds")
                total = sum(best) / 1e3
                line = {"set": name, "call": "panel_thin_depth R=%d" % R if R else "panel_thin", "n": len(f) + len(r),
                        "kept": int(out[0].sum()), "rounds": rounds, "first_gains": out[2][:5].tolist(),
                        "incidence_ms": best[0] / 1e3, "colsum_ms": best[1] / 1e3, "gain0_ms": best[2] / 1e3,
                        "rounds_ms": best[3] / 1e3, "us_per_round": round(best[3] / max(rounds, 1), 1),
                        "total_ms": round(total, 3)}
                if R:
                    line["shadows"] = eng.info("panel_thin_depth_shadows")
                    line["segments_all_ge_1_kept_ge_1_all_ge_R_kept_ge_R"] = out[5].tolist()
                    line["depth_all_sum"] = int(out[3].astype(np.int64).sum())
                    line["depth_kept_sum"] = int(out[4].astype(np.int64).sum())
                    line["vs_thin"] = round(total / thin_ms, 3)
                    line["colsum_over_incidence"] = round(best[1] / max(best[0], 1), 3)
                    if R == 1:
                        assert out[1].tolist() == thin_order and out[2].tolist() == thin_gains
                else:
                    thin_ms, thin_order, thin_gains = total, out[1].tolist(), out[2].tolist()
                    line["covered_all"], line["covered_kept"] = out[4], out[5]
                print(json.dumps(line), flush=True)
    finally:
        eng.device_free(hp)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
