"""Device time and outcome of the selection to a coverage depth (msspe_panel_select_depth_packed_dev) on the inputs of
tools/perf_panel_select.py: msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed form, segment 500 /
stride 250 / window 50, k 13, the string rule at up to 2 mismatches with the last 3 bases exact, min_gain 1, the
unfiltered stage-A winners of tests/golden/config2_10k.json (1,225; a word of both lists is kept once) under the
pool's screen at the ntthal chemistry and -9,000 cal/mol (msspe_cross_dimer_dev, bitmap only), T = 1 and 8, R = 1, 2
and 3.  In the same session, on the same inputs: msspe_panel_select_packed_dev at the same T, and
msspe_panel_thin_depth_packed_dev at the same R (it knows no conflicts).

    python tools/perf_panel_select_depth.py [--rows 10000] [--length 30000] [--reps 3]

The phases are the call's own device times between events on its stream (msspe_get_info "panel_select_prepare_us",
"panel_select_incidence_us", "panel_select_first_us", "panel_select_rounds_us", and "panel_select_depth_layer_us": the
column sums and every layer's init and first gains, which lie inside the last two), the best total of --reps calls
after one warm-up.  Prints one JSON line per call; "vs_select" is the call's device time over msspe_panel_select's at
the same T."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

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
    fwd = list(dict.fromkeys(w for w, _ in fx["winners"]["0"]))
    rev = [w for w in dict.fromkeys(w for w, _ in fx["winners"]["1"]) if w not in set(fwd)]
    g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
    n_seq, L = g.shape
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    hp = eng.put_rows_packed(g)
    opt = msspe_amd.KmerOpt(500, 250, 50, 13, 0, 0)
    M, E, thr = 2, 3, -9000.0
    chem, rule = msspe_amd.Chem.ntthal(), msspe_amd.seed_rule(M, E)
    aln = (hp, n_seq, L)
    f, r = msspe_amd.pack_oligos(fwd), msspe_amd.pack_oligos(rev)
    n, W = len(f) + len(r), (len(f) + len(r) + 63) // 64

    def put(a):
        dev = C.c_void_p()
        eng._check(eng.L.msspe_device_put(eng.ptr, a.ctypes.data, a.nbytes, C.byref(dev)))
        return int(dev.value)

    def best_of(*calls):
        """calls: (fn, info keys) pairs, run in turn --reps times after one warm-up round, so that two calls that are
        compared see the same neighbours; returns (last result, best phase times) per call, best by the sum of the
        first four."""
        best, out = [None] * len(calls), [None] * len(calls)
        for rep in range(args.reps + 1):
            for i, (fn, keys) in enumerate(calls):
                out[i] = fn()
                us = [eng.info(k) for k in keys]
                if rep and (best[i] is None or sum(us[:4]) < sum(best[i][:4])):
                    best[i] = us
        return list(zip(out, best))

    select_keys = ["panel_select_%s_us" % ph for ph in ("prepare", "incidence", "first", "rounds")]
    depth_keys = select_keys + ["panel_select_depth_layer_us"]
    thin_keys = ["panel_thin_%s_us" % ph for ph in ("incidence", "depth_colsum", "gain0", "rounds")]
    d_pool, d_bits = put(np.concatenate([f, r])), put(np.zeros((n, W), np.uint64))
    try:
        eng.cross_dimer_dev(d_pool, n, 13, chem, thr, (0, n), (0, n), d_bitmap=d_bits)
        bits = eng.device_get(d_bits, n * W * 8).view(np.uint64).reshape(n, W)
        edges = int(np.unpackbits(bits.view(np.uint8)).sum())
        for T in (1, 8):
            calls = [(lambda: eng.panel_select(aln, opt, f, r, rule, d_bits, T, form="packed"), select_keys)]
            calls += [(lambda R=R: eng.panel_select_depth(aln, opt, f, r, rule, R, d_bits, T, form="packed"),
                       depth_keys) for R in (1, 2, 3)]
            results = best_of(*calls)
            flat, us = results[0]
            rounds = int(flat["order"].size) + 1
            select_ms = sum(us) / 1e3
            select_round_us = us[3] / max(rounds, 1)
            print(json.dumps({"call": "panel_select", "n": n, "directed_edges": edges, "T": T,
                              "kept": int(flat["keep"].sum()), "barred": int(flat["barred"].sum()),
                              "tubes_used": flat["tubes_used"], "covered_all": flat["covered_all"],
                              "covered_kept": flat["covered_kept"], "segments": int(flat["covered"].size),
                              "prepare_ms": us[0] / 1e3, "incidence_ms": us[1] / 1e3, "first_ms": us[2] / 1e3,
                              "rounds_ms": us[3] / 1e3, "rounds": rounds, "us_per_round": round(select_round_us, 1),
                              "total_ms": round(select_ms, 3)}), flush=True)
            for R in (1, 2, 3):
                res, us = results[R]
                layers = int(res["layer"].max()) if res["layer"].size else 1
                rounds = int(res["order"].size) + layers
                total = sum(us[:4]) / 1e3
                if R == 1:
                    assert np.array_equal(res["order"], flat["order"]) and np.array_equal(res["gains"], flat["gains"])
                    assert np.array_equal(res["tube"], flat["tube"])
                print(json.dumps({"call": "panel_select_depth R=%d" % R, "n": n, "T": T,
                                  "kept": int(res["keep"].sum()), "layers": layers,
                                  "picks_per_layer": np.bincount(res["layer"], minlength=layers + 1)[1:].tolist(),
                                  "barred": int(res["barred"].sum()), "tubes_used": res["tubes_used"],
                                  "segments_all_ge_1_kept_ge_1_all_ge_R_kept_ge_R": res["counts"].tolist(),
                                  "prepare_ms": us[0] / 1e3, "incidence_ms": us[1] / 1e3, "first_ms": us[2] / 1e3,
                                  "rounds_ms": us[3] / 1e3, "layer_ms": us[4] / 1e3, "rounds": rounds,
                                  "us_per_round": round((us[2] + us[3] - us[4]) / max(rounds, 1), 1),
                                  "select_us_per_round": round(select_round_us, 1), "total_ms": round(total, 3),
                                  "vs_select": round(total / select_ms, 3)}), flush=True)
        for R in (1, 2, 3):
            (out, us), = best_of((lambda: eng.panel_thin_depth(aln, opt, f, r, M, E, R, form="packed"), thin_keys))
            rounds = eng.info("panel_thin_rounds")
            print(json.dumps({"call": "panel_thin_depth R=%d" % R, "n": n, "kept": int(out[0].sum()),
                              "segments_all_ge_1_kept_ge_1_all_ge_R_kept_ge_R": out[5].tolist(),
                              "incidence_ms": us[0] / 1e3, "colsum_ms": us[1] / 1e3, "gain0_ms": us[2] / 1e3,
                              "rounds_ms": us[3] / 1e3, "rounds": rounds,
                              "us_per_round": round(us[3] / max(rounds, 1), 1),
                              "total_ms": round(sum(us) / 1e3, 3)}), flush=True)
    finally:
        eng.device_free(d_pool)
        eng.device_free(d_bits)
        eng.device_free(hp)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
