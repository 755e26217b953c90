"""Device time of the target-reach call (msspe_stream_reach_packed_dev) beside its sibling, the scored screen
(msspe_background_thal_flank_packed_dev at flank 0) with the same arguments, same session, same device: a resident
stream of --records random records of --length columns (10,000 x 30 kb), the 572-primer kept panel
(tests/golden/config2_10k.json), k = 13, M = 2, E = 3, D = 500; once with the string rule (threshold 0) and once with
thal END1 at 30 C.

    python tools/perf_stream_reach.py [--records 10000] [--length 30000] [--reach 500] [--min-seconds 1.0]

The sibling's code is what it was before the reach call existed, so it is the baseline: what the reach call costs on
top is the cleared planes, the atomicOr of the fold and the five reach kernels.  Call figures are device time between
two events on the engine's stream, read after a synchronise, averaged over as many repetitions as make up
--min-seconds, after one warm-up call.  The per-kernel figures are the call's own events around each launch
(msspe_get_info reach_*_us) of the last repetition.  One JSON line per rule:
  thal_ms, reach_ms   the two calls; reach_over_thal their ratio
  tiles_us, scan_us (both scans), masks_us, gap_tiles_us, gaps_us   the new kernels
  masks_bytes         what the planes pass moves: it reads the plus and minus planes (the minus plane's words twice, one
                      word apart, the second time from cache) and writes the third: 3 x 8 bytes per 64 columns
  masks_gb_per_s      masks_bytes / masks_us, to hold beside the copy ceiling bench.py quotes
  pass_us, pass_bytes, pass_gb_per_s   all five kernels together: the tiles kernel reads two planes, the masks kernel
                      reads two and writes one, the gap kernels read the third once each: 7 x 8 bytes per 64 columns
Records of random bases hold no designed sites: the panel lands by chance, about one site per 135 columns or 220 per
record, the order of a designed panel on its own targets (a few hundred sites per genome)."""
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


def random_records(rng, n, length):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [acgt[rng.integers(0, 4, size=length, dtype=np.uint8)].tobytes() for _ in range(n)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--reach", type=int, default=500)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    panel = fx["primers_kept"]["F"] + fx["primers_kept"]["R"]
    k, M, E = 13, 2, 3
    chem = msspe_amd.Chem.ntthal()
    rng = np.random.default_rng(31)
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    d = None
    try:
        d, L, starts = eng.put_stream_packed(random_records(rng, args.records, args.length))
        words = msspe_amd.pack_oligos(panel)
        for rule, mode, thr in (("string", "any", 0.0), ("end1_30C", "end1", 30.0)):
            def thal():
                return eng.background_thal_packed(d, L, words, M, E, chem, thr, mode, k=k)

            def reach():
                return eng.stream_reach_packed(d, L, words, M, E, chem, thr, mode, args.reach, record_start=starts,
                                               k=k)

            counts, stable = thal()
            c2, s2, recs = reach()
            assert (c2 == counts).all() and (s2 == stable).all()
            t_thal = timed(torch, thal, args.min_seconds)
            t_reach = timed(torch, reach, args.min_seconds)
            us = {key: eng.info(f"reach_{key}_us") for key in ("tiles", "scan", "masks", "gap_tiles", "gaps")}
            masks_bytes = 3 * 8 * ((L + 63) // 64)
            pass_bytes, pass_us = 7 * 8 * ((L + 63) // 64), sum(us.values())
            print(json.dumps({
                "case": rule, "k": k, "records": args.records, "columns": L, "primers": len(panel),
                "reach": args.reach, "sites": int(counts.sum()), "stable": int(stable.sum()),
                "reached_either": int(recs["reached_either"].astype(np.int64).sum()),
                "slabs": eng.info("background_thal_slabs"), "plane_bytes": eng.info("reach_plane_bytes"),
                "thal_ms": round(t_thal * 1e3, 3), "reach_ms": round(t_reach * 1e3, 3),
                "reach_over_thal": round(t_reach / t_thal, 4),
                **{f"{key}_us": v for key, v in us.items()},
                "masks_bytes": masks_bytes,
                "masks_gb_per_s": round(masks_bytes / max(us["masks"], 1) / 1e3, 1),
                "pass_us": pass_us, "pass_bytes": pass_bytes,
                "pass_gb_per_s": round(pass_bytes / max(pass_us, 1) / 1e3, 1)}), flush=True)
    finally:
        if d is not None:
            eng.device_free(d)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
