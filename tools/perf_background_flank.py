"""Device time of the scored background screen with template flanks (msspe_background_thal_flank_packed_dev) beside the
same call at flank 0, same session, same device: a resident random stream of 2^--log2-columns columns, the 572-primer
kept panel (tests/golden/config2_10k.json), k = 13, M = 2, E = 3, 30 C, mode ANY.

    python tools/perf_background_flank.py [--log2-columns 28] [--min-seconds 1.0] [--flanks 0,1,2]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_background_flank.py --once 2

Every figure is device time between two events on the engine's stream, read after a synchronise, summed over as many
repetitions as make up --min-seconds, after one warm-up call (the calls copy their per-primer counts back and
synchronise: inside the figure).  One JSON line per case:
  site_list   msspe_background_sites_packed_dev with the site list: what finding the sites costs, the part of every
              scored call that does not depend on the flank
  scored      the scored call at one flank: sites/s of the whole call, sites/s of the scoring alone (the call minus
              site_list), the classes and truncated sites it reports, and both rates relative to flank 0
--once F runs one warm-up call and one measured call at flank F and nothing else: the run to put under
rocprofv3 --kernel-trace --stats, whose kernel table gives the share of k_site_oligos_flank and k_site_group."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))
sys.path.insert(0, str(ROOT / "tools"))
from perf_background import timed  # noqa: E402
from perf_background_thal import random_stream  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-columns", type=int, default=28)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--flanks", default="0,1,2")
    ap.add_argument("--once", type=int, default=None)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    panel = fx["primers_kept"]["F"] + fx["primers_kept"]["R"]
    k, M, E, thr = 13, 2, 3, 30.0
    chem = msspe_amd.Chem.ntthal()
    rng = np.random.default_rng(29)
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    d = None
    try:
        d, L, _ = eng.put_stream_packed(random_stream(rng, 1 << args.log2_columns))
        words = msspe_amd.pack_oligos(panel)

        def scored(f):
            return eng.background_thal_packed(d, L, words, M, E, chem, thr, "any", k=k, flank=f)

        if args.once is not None:
            scored(args.once)
            counts, stable = scored(args.once)
            print(json.dumps({"case": "once", "flank": args.once, "sites": int(counts.sum()),
                              "stable": int(stable.sum())}), flush=True)
            return
        counts = eng.background_sites_packed(d, L, words, M, E, k=k)
        n_sites = int(counts.sum())
        cap = n_sites + 1024
        d_sites = torch.zeros(cap * 12, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")

        def with_list():
            d_count.zero_()
            eng.background_sites_packed(d, L, words, M, E, k=k, d_sites=d_sites.data_ptr(), capacity=cap,
                                        d_count=d_count.data_ptr())
        t_list = timed(torch, with_list, args.min_seconds)
        print(json.dumps({"case": "site_list", "k": k, "columns": L, "primers": len(panel), "sites": n_sites,
                          "ms": round(t_list * 1e3, 3)}), flush=True)
        base = None
        for f in [int(x) for x in args.flanks.split(",")]:
            c, stable = scored(f)
            assert (c == counts).all()
            t = timed(torch, lambda: scored(f), args.min_seconds)
            call_rate, score_rate = n_sites / t, n_sites / (t - t_list)
            if base is None:
                base = (f, call_rate, score_rate)
            print(json.dumps({"case": "scored", "flank": f, "sites": n_sites, "stable": int(stable.sum()),
                              "classes": eng.info("background_thal_flank_classes"),
                              "truncated": eng.info("background_thal_truncated"),
                              "slabs": eng.info("background_thal_slabs"), "call_ms": round(t * 1e3, 3),
                              "call_sites_per_s": float("%.4g" % call_rate),
                              "scoring_sites_per_s": float("%.4g" % score_rate),
                              f"call_vs_flank_{base[0]}": round(call_rate / base[1], 3),
                              f"scoring_vs_flank_{base[0]}": round(score_rate / base[2], 3)}), flush=True)
    finally:
        if d is not None:
            eng.device_free(d)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
