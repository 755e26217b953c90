"""Device time of the scored background screen (msspe_background_thal_packed_dev) on a resident random stream, beside
the calls it is measured against, same session, same device, 572-primer kept panel (tests/golden/config2_10k.json),
M = 2, E = 3.

    python tools/perf_background_thal.py [--log2-columns 28] [--min-seconds 1.0] [--pool 4096] [--small-cap 16]

Every figure is device time between two events on the engine's stream, read after a synchronise, summed over as many
repetitions as make up --min-seconds, after one warm-up call (the calls copy their per-primer counts back and
synchronise: inside the figure).  Cases, one JSON line each:
  any_screen_f64   the f64 ANY screen (pair_kernel=f64) of a random pool of --pool oligos: checks/s, 13- and 20-mers
  scoring          the scored call minus the site-list call on the same stream (2^24 columns): what the site oligos,
                   the DP launches and the fold cost, as scored sites/s, and its ratio to the screen's checks/s
  whole_call       the scored call on 2^--log2-columns columns beside the counts-only call; scoring_share
  split            the same call through a work list of 2^--small-cap sites: slabs, splits and time"""
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


def random_stream(rng, total, n_rec=64):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [letters[rng.integers(0, 4, total // n_rec - 1, dtype=np.uint8)].tobytes() for _ in range(n_rec)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-columns", type=int, default=28)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--small-cap", type=int, default=16)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    panel = fx["primers_kept"]["F"] + fx["primers_kept"]["R"]
    M, E, thr = 2, 3, 30.0
    chem = msspe_amd.Chem.ntthal()
    rng = np.random.default_rng(29)
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    handles = []
    try:
        d24, L24, _ = eng.put_stream_packed(random_stream(rng, 1 << 24))
        handles.append(d24)
        for k in (13, 20):
            pool = msspe_amd.synth.pool_strings(msspe_amd.synth.random_pool(args.pool, k))
            eng.set_option("pair_kernel", "f64")
            t_any = timed(torch, lambda: eng.cross_dimer(pool, chem, -9000.0, want_dg=False), args.min_seconds)
            eng.set_option("pair_kernel", "auto")
            any_rate = args.pool ** 2 / t_any
            print(json.dumps({"case": "any_screen_f64", "k": k, "pool": args.pool, "ms": round(t_any * 1e3, 3),
                              "checks_per_s": float("%.4g" % any_rate)}), flush=True)
            words = msspe_amd.pack_oligos([(p + p)[:k] for p in panel])
            counts, stable = eng.background_thal_packed(d24, L24, words, M, E, chem, thr, "any", k=k)
            n_sites = int(counts.sum())
            cap = n_sites + 1024
            d_sites = torch.zeros(cap * 12, dtype=torch.uint8, device="cuda")
            d_count = torch.zeros(1, dtype=torch.int64, device="cuda")

            def with_list():
                d_count.zero_()
                eng.background_sites_packed(d24, L24, words, M, E, k=k, d_sites=d_sites.data_ptr(), capacity=cap,
                                            d_count=d_count.data_ptr())
            t_list = timed(torch, with_list, args.min_seconds)
            for mode in ("any", "end1"):
                t_thal = timed(torch, lambda: eng.background_thal_packed(d24, L24, words, M, E, chem, thr, mode, k=k),
                               args.min_seconds)
                rate = n_sites / (t_thal - t_list)
                print(json.dumps({"case": "scoring", "k": k, "mode": mode, "columns": L24, "sites": n_sites,
                                  "stable": int(stable.sum()), "call_ms": round(t_thal * 1e3, 3),
                                  "site_list_ms": round(t_list * 1e3, 3), "scored_sites_per_s": float("%.4g" % rate),
                                  "vs_any_screen_f64": round(rate / any_rate, 3)}), flush=True)
        d, L, _ = eng.put_stream_packed(random_stream(rng, 1 << args.log2_columns))
        handles.append(d)
        words = msspe_amd.pack_oligos(panel)
        counts, stable = eng.background_thal_packed(d, L, words, M, E, chem, thr, "any", k=13)
        t_bg = timed(torch, lambda: eng.background_sites_packed(d, L, words, M, E, k=13), args.min_seconds)
        t_thal = timed(torch, lambda: eng.background_thal_packed(d, L, words, M, E, chem, thr, "any", k=13),
                       args.min_seconds)
        print(json.dumps({"case": "whole_call", "k": 13, "columns": L, "primers": len(panel), "sites": int(counts.sum()),
                          "stable": int(stable.sum()), "counts_only_ms": round(t_bg * 1e3, 3),
                          "scored_ms": round(t_thal * 1e3, 3), "slabs": eng.info("background_thal_slabs"),
                          "scoring_share": round(1.0 - t_bg / t_thal, 3)}), flush=True)
        eng.set_option("site_list_cap_log2", args.small_cap)
        c2, s2 = eng.background_thal_packed(d, L, words, M, E, chem, thr, "any", k=13)
        assert (c2 == counts).all() and (s2 == stable).all()
        t_split = timed(torch, lambda: eng.background_thal_packed(d, L, words, M, E, chem, thr, "any", k=13),
                        args.min_seconds)
        print(json.dumps({"case": "split", "site_list_cap_log2": args.small_cap, "scored_ms": round(t_split * 1e3, 3),
                          "slabs": eng.info("background_thal_slabs"), "redone": eng.info("background_thal_redone"),
                          "vs_default": round(t_split / t_thal, 3)}), flush=True)
    finally:
        for h in handles:
            eng.device_free(h)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
