"""Device time of the thal-scored panel thinning (msspe_panel_thin_thal_packed_dev) at config2 size:
msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed form, segment 500 / stride 250 / window 50, M = 2,
E = 3, END1, threshold 30, min_gain 1, for the fixture's kept 572-primer panel (tests/golden/config2_10k.json, k = 13)
and a panel of the same size cut from the alignment's first row at --long-k (24), with thin_thal_unique 0 and 1 in one
session on one context, beside msspe_panel_thin_packed_dev and msspe_segment_coverage_thal_packed_dev on the same
inputs.

    python tools/perf_panel_thin_thal.py [--rows 10000] [--length 30000] [--long-k 24] [--repeats 3]

The phases are the call's own event times (msspe_get_info "panel_thin_thal_list_us" / "_unique_us" / "_score_us" /
"_fold_us" summed over its slabs, "panel_thin_gain0_us", "panel_thin_thal_rounds_us"), of the best of --repeats calls
by the host's clock after one warm-up; "call_ms" is that clock around the whole call, the upload of the primer words and
the copies back included.  "held_before" is the whole panel's held segments (*covered_all_out), "held_after" what
msspe_segment_coverage_thal_packed_dev finds held for the kept primers alone.
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


def best_of(repeats, call, info):
    best = None
    for rep in range(repeats + 1):   # the first call is the warm-up
        t0 = time.perf_counter()
        out = call()
        t = time.perf_counter() - t0
        got = info()
        if rep and (best is None or t < best[0]):
            best = (t, got, out)
    return best


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
            fw, rw = msspe_amd.pack_oligos(f), msspe_amd.pack_oligos(r)
            t, info, out = best_of(args.repeats, lambda: eng.panel_thin(aln, opt, fw, rw, M, E, form="packed"),
                                   lambda: [eng.info("panel_thin_%s_us" % ph) for ph in ("incidence", "gain0", "rounds")])
            print(json.dumps({"case": "panel_thin", "k": k, "n": len(f) + len(r), "kept": int(out[0].sum()),
                              "covered_all": out[4], "covered_kept": out[5], "call_ms": round(t * 1e3, 3),
                              "incidence_ms": info[0] / 1e3, "gain0_ms": info[1] / 1e3, "rounds_ms": info[2] / 1e3}),
                  flush=True)
            t, info, cov = best_of(args.repeats,
                                   lambda: eng.segment_coverage_thal(aln, opt, f, r, M, E, chem, "end1", 30.0,
                                                                     packed="packed"),
                                   lambda: {key: eng.info("coverage_thal_" + key) for key in
                                            ("matches", "slabs", "list_us", "score_us", "fold_us")})
            print(json.dumps({"case": "coverage_thal", "k": k, "n": len(f) + len(r),
                              "held": int((cov["held"] == 2).sum()), "matched": int((cov["held"] != 0).sum()),
                              "call_ms": round(t * 1e3, 3), "list_ms": info["list_us"] / 1e3,
                              "score_ms": info["score_us"] / 1e3, "fold_ms": info["fold_us"] / 1e3,
                              "matches": info["matches"], "slabs": info["slabs"]}), flush=True)
            outs = []
            for unique in (0, 1):
                eng.set_option("thin_thal_unique", unique)
                t, info, out = best_of(
                    args.repeats,
                    lambda: eng.panel_thin_thal(aln, opt, fw, rw, M, E, chem, "end1", 30.0, form="packed"),
                    lambda: {**{key: eng.info("panel_thin_thal_" + key) for key in
                                ("matches", "unique_pairs", "slabs", "redone", "list_us", "unique_us", "score_us",
                                 "fold_us", "rounds_us")},
                             "gain0_us": eng.info("panel_thin_gain0_us"), "rounds": eng.info("panel_thin_rounds")})
                keep = out[0]
                kf = [w for w, q in zip(f, keep[:len(f)]) if q]
                kr = [w for w, q in zip(r, keep[len(f):]) if q]
                after = eng.segment_coverage_thal(aln, opt, kf, kr, M, E, chem, "end1", 30.0, packed="packed")
                outs.append([np.asarray(x).tobytes() for x in out])
                dev = sum(info[key] for key in ("list_us", "unique_us", "score_us", "fold_us", "gain0_us", "rounds_us"))
                print(json.dumps({"case": "panel_thin_thal", "k": k, "unique": unique, "n": len(f) + len(r),
                                  "kept": int(keep.sum()), "segments": int(out[3].size), "held_before": out[4],
                                  "held_kept": out[5], "held_after": int((after["held"] == 2).sum()),
                                  "held_whole_set_by_coverage_thal": int((cov["held"] == 2).sum()),
                                  "call_ms": round(t * 1e3, 3), "device_ms": dev / 1e3, "list_ms": info["list_us"] / 1e3,
                                  "unique_ms": info["unique_us"] / 1e3, "score_ms": info["score_us"] / 1e3,
                                  "fold_ms": info["fold_us"] / 1e3, "gain0_ms": info["gain0_us"] / 1e3,
                                  "rounds_ms": info["rounds_us"] / 1e3, "rounds": info["rounds"],
                                  "matches": info["matches"], "pairs_scored": info["unique_pairs"],
                                  "slabs": info["slabs"], "redone": info["redone"]}), flush=True)
            print(json.dumps({"case": "unique_0_equals_1", "k": k, "equal": outs[0] == outs[1]}), flush=True)
    finally:
        eng.set_option("thin_thal_unique", 1)
        eng.device_free(hp)
        eng.close()


if __name__ == "__main__":
    main()
