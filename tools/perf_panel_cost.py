"""Device time and outcome of the thinning and selection by gain per cost (msspe_panel_thin_cost_packed_dev,
msspe_panel_select_cost_packed_dev) beside their weighted and unweighted siblings, in one session at config2 size:
msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed form, segment 500 / stride 250 / window 50, k 13, the
string rule at up to 2 mismatches with the last 3 bases exact, min_gain 1.  Two cases over tests/golden/config2_10k.json:
the thinning of the 572 kept primers, and the selection of the 1,225 unfiltered stage-A winners (a word of both lists
kept once) at T = 1 and 8 over the pool's screen at the ntthal chemistry and -9,000 cal/mol.

    python tools/perf_panel_cost.py [--rows 10000] [--length 30000] [--seconds 1.0] [--out FILE]

Six calls alternate, call after call, after one warm-up each, until every one of them has been timed for at least
--seconds of device time (and three times): the unweighted sibling, the weighted sibling at weights 1 + (r % 7), the
cost call with all costs 1 without weights and with those weights, and the cost call with costs 1 + (p % 5) without
weights and with them.  Every figure is the call's own device time between events on its stream (msspe_get_info
"panel_thin_*_us", "panel_select_*_us"); a figure is the median over its calls, "spread" the lowest and highest total.
The incidence pass and the gains are the sibling's, so a cost call may differ from its sibling in "rounds" only.  The
all-ones cost calls are asserted equal to their siblings in every output and in the rounds run (guarantee 1 on the
real inputs).  Prints one JSON line per case and call."""
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
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import msspe_amd

    if not torch.cuda.is_available():
        raise SystemExit("perf_panel_cost: no GPU; nothing is measured without one")
    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
    n_seq, L = g.shape
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    hp = eng.put_rows_packed(g)
    opt = msspe_amd.KmerOpt(500, 250, 50, 13, 0, 0)
    P = (L - 500) // 250 + 1
    w = np.repeat((1 + np.arange(n_seq) % 7).astype(np.uint32), P)
    M, E, thr = 2, 3, -9000.0
    chem, rule = msspe_amd.Chem.ntthal(), msspe_amd.seed_rule(M, E)
    aln = (hp, n_seq, L)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def put(a):
        dev = C.c_void_p()
        eng._check(eng.L.msspe_device_put(eng.ptr, a.ctypes.data, a.nbytes, C.byref(dev)))
        return int(dev.value)

    def alternate(calls, keys, rounds_key):
        """calls: name -> function.  Returns name -> (last result, median per key, (lowest, highest) total, calls,
        rounds of the last call)."""
        times = {name: [] for name in calls}
        out, rounds = {}, {}
        for name, fn in calls.items():   # warm-up
            fn()
        while any(len(t) < 3 or sum(sum(x) for x in t) < args.seconds * 1e6 for t in times.values()):
            for name, fn in calls.items():
                out[name] = fn()
                times[name].append([eng.info(k) for k in keys])
                rounds[name] = eng.info(rounds_key)
        res = {}
        for name, t in times.items():
            a = np.array(t, dtype=np.float64)
            tot = a.sum(axis=1)
            res[name] = (out[name], np.median(a, axis=0), (float(tot.min()), float(tot.max())), len(t), rounds[name])
        return res

    thin_keys = ["panel_thin_%s_us" % ph for ph in ("incidence", "gain0", "rounds")]
    select_keys = ["panel_select_%s_us" % ph for ph in ("prepare", "incidence", "first", "rounds")]
    try:
        # the thinning of the 572 kept primers
        f, r = msspe_amd.pack_oligos(fx["primers_kept"]["F"]), msspe_amd.pack_oligos(fx["primers_kept"]["R"])
        n = len(f) + len(r)
        ones, mod5 = np.ones(n, np.uint32), (1 + np.arange(n) % 5).astype(np.uint32)
        calls = {"unweighted": lambda: eng.panel_thin(aln, opt, f, r, M, E, form="packed"),
                 "weighted": lambda: eng.panel_thin_weighted(aln, opt, f, r, M, E, w, form="packed"),
                 "cost_ones": lambda: eng.panel_thin_cost(aln, opt, f, r, M, E, ones, form="packed"),
                 "cost_ones_weighted": lambda: eng.panel_thin_cost(aln, opt, f, r, M, E, ones, w, form="packed"),
                 "cost_1+p%5": lambda: eng.panel_thin_cost(aln, opt, f, r, M, E, mod5, form="packed"),
                 "cost_1+p%5_weighted": lambda: eng.panel_thin_cost(aln, opt, f, r, M, E, mod5, w, form="packed")}
        res = alternate(calls, thin_keys, "panel_thin_rounds")
        for a, b in (("cost_ones", "unweighted"), ("cost_ones_weighted", "weighted")):
            assert all(np.array_equal(x, y) for x, y in zip(res[a][0][:len(res[b][0])], res[b][0])), (a, "differs from", b)
            assert res[a][4] == res[b][4], (a, "ran other rounds than", b)
        for name, (out, med, spread, count, rounds) in res.items():
            emit({"case": "thin_572", "call": name, "n": n, "segments": n_seq * P, "incidence_ms": med[0] / 1e3,
                  "gain0_ms": med[1] / 1e3, "rounds_ms": med[2] / 1e3, "total_ms": float(med.sum()) / 1e3,
                  "spread_ms": [spread[0] / 1e3, spread[1] / 1e3], "calls": count, "rounds": rounds,
                  "round_us": med[2] / rounds, "picks": int(out[1].size), "kept": int(out[0].sum()),
                  "covered_all": out[4], "covered_kept": out[5], "weight_kept": out[7] if len(out) > 6 else None,
                  "cost_all": out[8] if len(out) > 8 else None, "cost_kept": out[9] if len(out) > 8 else None})
        # the selection of the stage-A winners
        fwd = list(dict.fromkeys(x for x, _ in fx["winners"]["0"]))
        rev = [x for x in dict.fromkeys(x for x, _ in fx["winners"]["1"]) if x not in set(fwd)]
        f, r = msspe_amd.pack_oligos(fwd), msspe_amd.pack_oligos(rev)
        n, W = len(f) + len(r), (len(f) + len(r) + 63) // 64
        ones, mod5 = np.ones(n, np.uint32), (1 + np.arange(n) % 5).astype(np.uint32)
        d_pool, d_bits = put(np.concatenate([f, r])), put(np.zeros((n, W), np.uint64))
        try:
            eng.cross_dimer_dev(d_pool, n, 13, chem, thr, (0, n), (0, n), d_bitmap=d_bits)
            for T in (1, 8):
                sel = lambda c, wt=None: eng.panel_select_cost(aln, opt, f, r, rule, c, wt, d_bits, T, form="packed")
                calls = {"unweighted": lambda: eng.panel_select(aln, opt, f, r, rule, d_bits, T, form="packed"),
                         "weighted": lambda: eng.panel_select_weighted(aln, opt, f, r, rule, w, d_bits, T, form="packed"),
                         "cost_ones": lambda: sel(ones), "cost_ones_weighted": lambda: sel(ones, w),
                         "cost_1+p%5": lambda: sel(mod5), "cost_1+p%5_weighted": lambda: sel(mod5, w)}
                res = alternate(calls, select_keys, "panel_select_rounds")
                for a, b in (("cost_ones", "unweighted"), ("cost_ones_weighted", "weighted")):
                    assert all(np.array_equal(res[a][0][k], v) for k, v in res[b][0].items()), (a, "differs from", b)
                    assert res[a][4] == res[b][4], (a, "ran other rounds than", b)
                for name, (out, med, spread, count, rounds) in res.items():
                    emit({"case": "select_1225", "T": T, "call": name, "n": n, "segments": n_seq * P,
                          "prepare_ms": med[0] / 1e3, "incidence_ms": med[1] / 1e3, "first_ms": med[2] / 1e3,
                          "rounds_ms": med[3] / 1e3, "total_ms": float(med.sum()) / 1e3,
                          "spread_ms": [spread[0] / 1e3, spread[1] / 1e3], "calls": count, "rounds": rounds,
                          "round_us": med[3] / rounds, "picks": int(out["order"].size), "kept": int(out["keep"].sum()),
                          "barred": int(out["barred"].sum()), "tubes_used": out["tubes_used"],
                          "covered_all": out["covered_all"], "covered_kept": out["covered_kept"],
                          "weight_kept": out.get("weight_kept"), "cost_all": out.get("cost_all"),
                          "cost_kept": out.get("cost_kept")})
        finally:
            eng.device_free(d_pool)
            eng.device_free(d_bits)
    finally:
        eng.device_free(hp)
        eng.reset_stream()
        eng.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
