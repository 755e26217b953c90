"""Device time and outcome of the weighted thinning and selection (msspe_panel_thin_weighted_packed_dev,
msspe_panel_select_weighted_packed_dev) beside their unweighted siblings, in one session at config2 size:
msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed form, segment 500 / stride 250 / window 50, k 13, the
string rule at up to 2 mismatches with the last 3 bases exact, min_gain 1, under three weightings of the genomes --
all ones, 1 + (r % 7), and every tenth genome at weight 0 (the others 1).  Two cases over tests/golden/config2_10k.json:
the thinning of the 572 kept primers, and the selection of the 1,225 unfiltered stage-A winners (a word of both lists
kept once) at T = 1 and 8 over the pool's screen at the ntthal chemistry and -9,000 cal/mol.

    python tools/perf_panel_weighted.py [--rows 10000] [--length 30000] [--seconds 1.0] [--out FILE]

Every figure is the call's own device time between events on its stream (msspe_get_info "panel_thin_*_us",
"panel_select_*_us").  The unweighted call and the three weighted ones alternate, call after call, after one warm-up
each, until every one of them has been timed for at least --seconds of device time (and three times); a figure is the
median over its calls, "spread" the lowest and highest total.  The incidence pass is shared, so a weighted call may
differ from its sibling in "first" / "gain0" and "rounds" only.  Prints one JSON line per case and weighting."""
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
        raise SystemExit("perf_panel_weighted: no GPU; nothing is measured without one")
    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
    n_seq, L = g.shape
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    hp = eng.put_rows_packed(g)
    opt = msspe_amd.KmerOpt(500, 250, 50, 13, 0, 0)
    P = (L - 500) // 250 + 1
    rows = np.arange(n_seq)
    weightings = {"ones": np.ones(n_seq, np.uint32), "1+r%7": (1 + rows % 7).astype(np.uint32),
                  "tenth_zero": (rows % 10 != 0).astype(np.uint32)}
    weightings = {k: np.repeat(v, P) for k, v in weightings.items()}
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

    def alternate(calls, keys):
        """calls: name -> function.  Returns name -> (last result, median per key, (lowest, highest) total, calls)."""
        times = {name: [] for name in calls}
        out = {}
        for name, fn in calls.items():   # warm-up
            fn()
        while any(len(t) < 3 or sum(sum(x) for x in t) < args.seconds * 1e6 for t in times.values()):
            for name, fn in calls.items():
                out[name] = fn()
                times[name].append([eng.info(k) for k in keys])
        res = {}
        for name, t in times.items():
            a = np.array(t, dtype=np.float64)
            tot = a.sum(axis=1)
            res[name] = (out[name], np.median(a, axis=0), (float(tot.min()), float(tot.max())), len(t))
        return res

    thin_keys = ["panel_thin_%s_us" % ph for ph in ("incidence", "gain0", "rounds")]
    select_keys = ["panel_select_%s_us" % ph for ph in ("prepare", "incidence", "first", "rounds")]
    try:
        # the thinning of the 572 kept primers
        f, r = msspe_amd.pack_oligos(fx["primers_kept"]["F"]), msspe_amd.pack_oligos(fx["primers_kept"]["R"])
        calls = {"unweighted": lambda: eng.panel_thin(aln, opt, f, r, M, E, form="packed")}
        for name, w in weightings.items():
            calls[name] = lambda w=w: eng.panel_thin_weighted(aln, opt, f, r, M, E, w, form="packed")
        res = alternate(calls, thin_keys)
        plain = res["unweighted"][0]
        ones = res["ones"][0]
        assert all(np.array_equal(a, b) for a, b in zip(ones[:6], plain)), "all ones differ from the unweighted call"
        for name, (out, med, spread, count) in res.items():
            emit({"case": "thin_572", "weights": name, "n": len(f) + len(r), "segments": n_seq * P,
                  "incidence_ms": med[0] / 1e3, "gain0_ms": med[1] / 1e3, "rounds_ms": med[2] / 1e3,
                  "total_ms": float(med.sum()) / 1e3, "spread_ms": [spread[0] / 1e3, spread[1] / 1e3], "calls": count,
                  "picks": int(out[1].size), "kept": int(out[0].sum()), "covered_all": out[4], "covered_kept": out[5],
                  "weight_all": out[6] if len(out) > 6 else None, "weight_kept": out[7] if len(out) > 6 else None})
        # the selection of the stage-A winners
        fwd = list(dict.fromkeys(w for w, _ in fx["winners"]["0"]))
        rev = [w for w in dict.fromkeys(w for w, _ in fx["winners"]["1"]) if w not in set(fwd)]
        f, r = msspe_amd.pack_oligos(fwd), msspe_amd.pack_oligos(rev)
        n, W = len(f) + len(r), (len(f) + len(r) + 63) // 64
        d_pool, d_bits = put(np.concatenate([f, r])), put(np.zeros((n, W), np.uint64))
        try:
            eng.cross_dimer_dev(d_pool, n, 13, chem, thr, (0, n), (0, n), d_bitmap=d_bits)
            for T in (1, 8):
                calls = {"unweighted": lambda: eng.panel_select(aln, opt, f, r, rule, d_bits, T, form="packed")}
                for name, w in weightings.items():
                    calls[name] = lambda w=w: eng.panel_select_weighted(aln, opt, f, r, rule, w, d_bits, T,
                                                                         form="packed")
                res = alternate(calls, select_keys)
                plain, ones = res["unweighted"][0], res["ones"][0]
                assert all(np.array_equal(ones[k], v) for k, v in plain.items()), "all ones differ from the unweighted call"
                for name, (out, med, spread, count) in res.items():
                    emit({"case": "select_1225", "T": T, "weights": name, "n": n, "segments": n_seq * P,
                          "prepare_ms": med[0] / 1e3, "incidence_ms": med[1] / 1e3, "first_ms": med[2] / 1e3,
                          "rounds_ms": med[3] / 1e3, "total_ms": float(med.sum()) / 1e3,
                          "spread_ms": [spread[0] / 1e3, spread[1] / 1e3], "calls": count,
                          "picks": int(out["order"].size), "kept": int(out["keep"].sum()),
                          "barred": int(out["barred"].sum()), "tubes_used": out["tubes_used"],
                          "covered_all": out["covered_all"], "covered_kept": out["covered_kept"],
                          "weight_all": out.get("weight_all"), "weight_kept": out.get("weight_kept")})
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
