"""Device time of the thal-scored coverage (msspe_segment_coverage_thal_packed_dev) beside coverage within N mismatches
with counts (msspe_segment_coverage_mm_packed_dev) at config2 size: msspe_amd.synth.aligned_genomes(10000, 30000)
resident in packed form, the fixture's kept 572-primer panel (tests/golden/config2_10k.json), segment 500 / stride 250 /
window 50, M = 2, E = 3, END1, threshold 30, in one session on one device.

    python tools/perf_coverage_thal.py [--rows 10000] [--length 30000] [--long-k 24] [--repeats 3]

The phases are the call's own event times (msspe_get_info "coverage_thal_list_us" / "_score_us" / "_fold_us", summed
over its slabs), the best of --repeats calls after one warm-up; "call_ms" is the host's clock around the whole call,
uploads of the primer words and the copies back included.  The mm line is timed the same way around its call.  One
more call with the record list gives the number of distinct (primer, template) pairs among the matches -- thal is a
pure function of the pair, so matches / distinct is what scoring each pair once would save.  The long length (a panel
of the same size cut from the alignment's first row) takes the one-wave-per-pair kernel.
Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--long-k", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    fwd13, rev13 = fx["primers_kept"]["F"], fx["primers_kept"]["R"]
    g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
    n, L = g.shape
    seg, stride, W, M, E = 500, 250, 50, 2, 3
    rng = np.random.default_rng(24)
    kl = args.long_k
    row = bytes(g[0]).decode()
    starts = [c for c in rng.integers(0, L - kl, 4 * len(fwd13)) if set(row[c:c + kl]) <= set("ACGT")]
    comp = str.maketrans("ACGT", "TGCA")
    fwd_l = [row[c:c + kl] for c in starts[:len(fwd13)]]
    rev_l = [row[c:c + kl].translate(comp)[::-1] for c in starts[len(fwd13):len(fwd13) + len(rev13)]]
    chem = msspe_amd.Chem.ntthal()
    eng = msspe_amd.Engine(0)
    hp = eng.put_rows_packed(g)
    aln = (hp, n, L)
    try:
        for k, f, r in ((13, fwd13, rev13), (kl, fwd_l, rev_l)):
            opt = msspe_amd.KmerOpt(seg, stride, W, k, 0, 0)
            best = None
            for rep in range(args.repeats + 1):   # the first call is the warm-up
                t0 = time.perf_counter()
                eng.segment_coverage_mm_packed(hp, n, L, opt, f, r, M, E, per_primer=True)
                t = time.perf_counter() - t0
                if rep and (best is None or t < best):
                    best = t
            print(json.dumps({"case": "mm_counts", "k": k, "primers": len(f) + len(r), "call_ms": round(best * 1e3, 3)}),
                  flush=True)
            best = None
            for rep in range(args.repeats + 1):
                t0 = time.perf_counter()
                out = eng.segment_coverage_thal(aln, opt, f, r, M, E, chem, "end1", 30.0, packed="packed")
                t = time.perf_counter() - t0
                info = {key: eng.info("coverage_thal_" + key) for key in
                        ("matches", "slabs", "redone", "list_us", "score_us", "fold_us")}
                if rep and (best is None or t < best[0]):
                    best = (t, info)
            t, info = best
            line = {"case": "thal", "k": k, "primers": len(f) + len(r), "segments": int(out["held"].size),
                    "matched": int((out["held"] != 0).sum()), "held": int((out["held"] == 2).sum()),
                    "call_ms": round(t * 1e3, 3), "list_ms": info["list_us"] / 1e3, "score_ms": info["score_us"] / 1e3,
                    "fold_ms": info["fold_us"] / 1e3, "matches": info["matches"], "slabs": info["slabs"],
                    "redone": info["redone"],
                    "matches_per_s": float("%.4g" % (info["matches"] / max(info["score_us"], 1) * 1e6))}
            recs = eng.segment_coverage_thal(aln, opt, f, r, M, E, chem, "end1", 30.0, matches=True,
                                             packed="packed")["matches"]
            # the template is the match's k columns (its orientation is fixed by the primer's direction), so the
            # distinct (primer, columns) rows are the distinct (primer, template) pairs
            P = out["held"].shape[1]
            rows, part = recs["segment"].astype(np.int64) // P, recs["segment"].astype(np.int64) % P
            col = part * stride + np.where(recs["primer"] >= len(f), seg - W, 0) + recs["offset"].astype(np.int64)
            cols = g[rows[:, None], col[:, None] + np.arange(k)[None, :]]
            key = np.concatenate([recs["primer"].astype("<u4").view(np.uint8).reshape(-1, 4), cols], axis=1)
            line["distinct_pairs"] = int(len(np.unique(np.ascontiguousarray(key).view(f"V{k + 4}"))))
            print(json.dumps(line), flush=True)
    finally:
        eng.device_free(hp)
        eng.close()


if __name__ == "__main__":
    main()
