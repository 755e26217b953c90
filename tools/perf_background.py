"""Device time of the background screen (msspe_background_sites_packed_dev) on a resident random stream, beside the
call it is measured against: msspe_segment_coverage_mm_packed_dev with per-primer counts at config2 size,
same session, same device, same 572-primer kept panel (tests/golden/config2_10k.json), M = 2, E = 3, k = 13.

    python tools/perf_background.py [--log2-columns 28] [--min-seconds 1.0] [--rows 10000] [--length 30000]

Every figure is device time between two events on the engine's stream, read after a synchronise, summed over as many
repetitions as make up --min-seconds, after one warm-up call (both calls copy their per-primer counts back to the host
and synchronise: that copy is inside the figure).  Background comparisons = 2 x stream columns x primers (both strands);
coverage comparisons = window positions x primers of their direction.  The site-list case runs at the hit density the
random stream gives at M = 2, E = 3 (reported as sites per million comparisons).  upload_pack is the host wall time of
msspe_device_put_stream_packed for the same stream held as 64 records.  Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))


def timed(torch, fn, min_seconds):
    fn()
    torch.cuda.synchronize()
    total, reps = 0.0, 0
    while total < min_seconds * 1000.0:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
        reps += 1
    return total / reps / 1000.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-columns", type=int, default=28)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    fwd, rev = fx["primers_kept"]["F"], fx["primers_kept"]["R"]
    panel = fwd + rev
    k, M, E = 13, 2, 3
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(28)
    total = 1 << args.log2_columns
    n_rec = 64
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    records = [letters[rng.integers(0, 4, total // n_rec - 1, dtype=np.uint8)].tobytes() for _ in range(n_rec)]
    t0 = time.perf_counter()
    d, L, _starts = eng.put_stream_packed(records)
    t_up = time.perf_counter() - t0
    print(json.dumps({"case": "upload_pack", "columns": L, "records": n_rec, "s": round(t_up, 3),
                      "GB_per_s": round(L / t_up / 1e9, 2)}), flush=True)
    hp = None
    try:
        # the yardstick: coverage within N mismatches with per-primer counts, config2 size
        g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
        hp = eng.put_rows_packed(g)
        n, glen = g.shape
        seg, stride, W = 500, 250, 50
        P = (glen - seg) // stride + 1
        opt = msspe_amd.KmerOpt(seg, stride, W, k, 0, 0)
        t_cov = timed(torch, lambda: eng.segment_coverage_mm_packed(hp, n, glen, opt, fwd, rev, M, E, per_primer=True),
                      args.min_seconds)
        cov_cmp = n * P * (W - k + 1) * len(panel)
        cov_rate = cov_cmp / t_cov
        print(json.dumps({"case": "coverage_mm_counts", "k": k, "M": M, "E": E, "primers": len(panel),
                          "ms": round(t_cov * 1e3, 3), "comparisons": cov_cmp,
                          "comparisons_per_s": float("%.4g" % cov_rate)}), flush=True)
        words = msspe_amd.pack_oligos(panel)
        bg_cmp = 2 * L * len(panel)
        counts = eng.background_sites_packed(d, L, words, M, E, k=k)
        n_sites = int(counts.sum())
        t_bg = timed(torch, lambda: eng.background_sites_packed(d, L, words, M, E, k=k), args.min_seconds)
        rate = bg_cmp / t_bg
        print(json.dumps({"case": "background_counts", "k": k, "M": M, "E": E, "primers": len(panel), "columns": L,
                          "ms": round(t_bg * 1e3, 3), "comparisons": bg_cmp, "sites": n_sites,
                          "comparisons_per_s": float("%.4g" % rate), "vs_coverage_mm_counts": round(rate / cov_rate, 3)}),
              flush=True)
        cap = n_sites + 1024
        d_sites = torch.zeros(cap * 12, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")

        def with_list():
            d_count.zero_()
            eng.background_sites_packed(d, L, words, M, E, k=k, d_sites=d_sites.data_ptr(), capacity=cap,
                                        d_count=d_count.data_ptr())
        t_list = timed(torch, with_list, args.min_seconds)
        assert int(d_count.item()) == n_sites
        print(json.dumps({"case": "background_list", "k": k, "M": M, "E": E, "ms": round(t_list * 1e3, 3),
                          "sites": n_sites, "sites_per_million_comparisons": round(n_sites / bg_cmp * 1e6, 3),
                          "comparisons_per_s": float("%.4g" % (bg_cmp / t_list))}), flush=True)
        k24 = [(p + p)[:24] for p in panel]
        w24 = msspe_amd.pack_oligos(k24)
        t24 = timed(torch, lambda: eng.background_sites_packed(d, L, w24, M, E, k=24), args.min_seconds)
        print(json.dumps({"case": "background_counts", "k": 24, "M": M, "E": E, "primers": len(k24), "columns": L,
                          "ms": round(t24 * 1e3, 3), "comparisons_per_s": float("%.4g" % (bg_cmp / t24))}), flush=True)
    finally:
        eng.device_free(d)
        if hp is not None:
            eng.device_free(hp)
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
