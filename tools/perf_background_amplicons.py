"""Device time of the off-target amplicon call (msspe_background_amplicons_packed_dev) beside the scored call it rides
on (msspe_background_thal_packed_dev, the same arguments, the same engine and session): the resident random stream of
2^--log2-columns columns in 64 records and the 572-primer kept panel (tests/golden/config2_10k.json) that
tools/perf_background_thal.py uses, M = 2, E = 3, thal ANY, product lengths --min-len .. --max-len.

    python tools/perf_background_amplicons.py [--log2-columns 28] [--min-seconds 1.0] [--min-len 50] [--max-len 1000]

Every call figure is device time between two events on the engine's stream, read after a synchronise, averaged over
as many repetitions as make up --min-seconds, after one warm-up call (the calls copy their counts back and synchronise:
inside the figure).  One JSON line per threshold, 30 C (what a user would pick) and 0 (every site stable, the dense
case):
  scored_ms        msspe_background_thal_packed_dev
  amplicons_ms     msspe_background_amplicons_packed_dev, counts only; added_ms = the difference
  sort_ms, join_ms the call's own HIP events around the key sort with the record ids, and around the join
                   (msspe_get_info "amplicon_sort_us" / "amplicon_join_us", of the last repetition)
  keys_ms          added_ms - sort_ms - join_ms: the key sink of the fold, the buffer's growth and the host's part
  with_list_ms     the same call appending every amplicon to a device list
  keys, amplicons  stable keys joined and amplicons found; key_grows: doublings of the key buffer"""
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
    ap.add_argument("--min-len", type=int, default=50)
    ap.add_argument("--max-len", type=int, default=1000)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    panel = fx["primers_kept"]["F"] + fx["primers_kept"]["R"]
    M, E = 2, 3
    chem = msspe_amd.Chem.ntthal()
    rng = np.random.default_rng(29)
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    d = None
    try:
        d, L, starts = eng.put_stream_packed(random_stream(rng, 1 << args.log2_columns))
        words = msspe_amd.pack_oligos(panel)
        for thr in (30.0, 0.0):
            def scored():
                return eng.background_thal_packed(d, L, words, M, E, chem, thr, "any", k=13)

            def joined(**kw):
                return eng.background_amplicons_packed(d, L, words, M, E, chem, thr, "any", args.min_len, args.max_len,
                                                       record_start=starts, k=13, **kw)
            counts, stable = scored()
            c2, s2, amp, total = joined()
            assert (c2 == counts).all() and (s2 == stable).all() and int(amp[:, 0].sum()) == int(amp[:, 1].sum()) == total
            t_thal = timed(torch, scored, args.min_seconds)
            t_amp = timed(torch, joined, args.min_seconds)
            sort_ms, join_ms = eng.info("amplicon_sort_us") / 1e3, eng.info("amplicon_join_us") / 1e3
            keys, grows = eng.info("amplicon_keys"), eng.info("amplicon_key_grows")
            cap = total + 1024
            d_list = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
            d_count = torch.zeros(1, dtype=torch.int64, device="cuda")

            def listed():
                d_count.zero_()
                joined(d_amplicons=d_list.data_ptr(), capacity=cap, d_count=d_count.data_ptr())
            t_list = timed(torch, listed, args.min_seconds)
            assert int(d_count.item()) == total
            added = (t_amp - t_thal) * 1e3
            print(json.dumps({"case": "amplicons", "tm_threshold": thr, "columns": L, "primers": len(panel),
                              "len": [args.min_len, args.max_len], "sites": int(counts.sum()), "keys": keys,
                              "amplicons": total, "key_grows": grows, "scored_ms": round(t_thal * 1e3, 3),
                              "amplicons_ms": round(t_amp * 1e3, 3), "added_ms": round(added, 3),
                              "sort_ms": round(sort_ms, 3), "join_ms": round(join_ms, 3),
                              "keys_ms": round(added - sort_ms - join_ms, 3), "with_list_ms": round(t_list * 1e3, 3),
                              "added_share": round(added / (t_thal * 1e3), 4)}), flush=True)
            del d_list
    finally:
        if d is not None:
            eng.device_free(d)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
