"""Device time of the reach thinning (msspe_panel_thin_reach_packed_dev) beside the call it grew from, the reach report
(msspe_stream_reach_packed_dev) with the same arguments, same session, same device, at two shapes:
  random    tools/perf_stream_reach.py's: --records random records of --length columns (10,000 x 30 kb);
  synthetic the ungapped rows of msspe_amd.synth.aligned_genomes(--records, --length), the alignment the panel was
            designed on.
The panel is the 572-primer kept panel (tests/golden/config2_10k.json), k = 13, M = 2, E = 3, D = 500, min_gain 1,
nothing forced; the string rule (threshold 0) on both shapes, thal END1 at 30 C on the random one as well.

    python tools/perf_panel_thin_reach.py [--records 10000] [--length 30000] [--reach 500] [--min-seconds 1.0]
                                          [--shapes random,synthetic]

The two calls ALTERNATE, each between two events on the engine's stream read after a synchronise, until each has at
least --min-seconds of device time; the figures are medians over the repetitions, after one warm-up call each.  The
phases are the call's own events (msspe_get_info thin_reach_*_us) of the last repetition.  One JSON line per case:
  reach_ms, thin_ms            the two calls; thin_over_reach their ratio
  sites, intervals             stable keys, and the disjoint intervals they leave
  rounds, kept, primers        rounds that ran (picks + 1), kept / n
  prepare_us, gain0_us, rounds_us, report_us   the phases behind the scored pass; round_us = rounds_us / rounds
  plane_words                  words of the covered plane a round's rank pass reads"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))


def random_records(rng, n, length):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [acgt[rng.integers(0, 4, size=length, dtype=np.uint8)].tobytes() for _ in range(n)]


def alternate(torch, fns, min_seconds):
    """Median device milliseconds of each fn, the calls taking turns until each has min_seconds of device time."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    while min(sum(t) for t in times) < min_seconds * 1000.0:
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1))
    return [statistics.median(t) for t in times], len(times[0])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--reach", type=int, default=500)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--shapes", default="random,synthetic")
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    panel = fx["primers_kept"]["F"] + fx["primers_kept"]["R"]
    k, M, E = 13, 2, 3
    chem = msspe_amd.Chem.ntthal()
    words = msspe_amd.pack_oligos(panel)
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for shape in args.shapes.split(","):
            if shape == "random":
                records = random_records(np.random.default_rng(31), args.records, args.length)
                rules = (("string", "any", 0.0), ("end1_30C", "end1", 30.0))
            else:
                g = msspe_amd.synth.aligned_genomes(args.records, args.length)
                records = [r[r != ord("-")].tobytes() for r in g]
                rules = (("string", "any", 0.0),)
            d, L, starts = eng.put_stream_packed(records)
            del records
            try:
                for rule, mode, thr in rules:
                    def reach():
                        return eng.stream_reach_packed(d, L, words, M, E, chem, thr, mode, args.reach,
                                                       record_start=starts, k=k)

                    def thin():
                        return eng.panel_thin_reach_packed(d, L, words, M, E, chem, thr, mode, args.reach,
                                                           record_start=starts, k=k)

                    counts, stable, recs = reach()
                    res = thin()
                    assert (res["counts"] == counts).all() and (res["stable"] == stable).all()
                    assert res["reached_kept"] == res["reached_all"] == int(recs["reached_either"].astype(np.int64).sum())
                    assert (res["records"]["reached_either"] == recs["reached_either"]).all()
                    (t_reach, t_thin), reps = alternate(torch, (reach, thin), args.min_seconds)
                    us = {key: eng.info(f"thin_reach_{key}_us") for key in ("prepare", "gain0", "rounds", "report")}
                    rounds = eng.info("thin_reach_rounds")
                    print(json.dumps({
                        "shape": shape, "case": rule, "k": k, "records": args.records, "columns": L,
                        "primers": len(panel), "reach": args.reach, "sites": int(counts.sum()),
                        "stable": eng.info("thin_reach_sites"), "intervals": eng.info("thin_reach_intervals"),
                        "reached": res["reached_all"], "kept": int(res["keep"].sum()), "rounds": rounds,
                        "repetitions": reps, "reach_ms": round(t_reach, 3), "thin_ms": round(t_thin, 3),
                        "thin_over_reach": round(t_thin / t_reach, 4),
                        **{f"{key}_us": v for key, v in us.items()},
                        "round_us": round(us["rounds"] / max(rounds, 1), 1),
                        "plane_words": (L + 63) // 64}), flush=True)
            finally:
                eng.device_free(d)
    finally:
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
