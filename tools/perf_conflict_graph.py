"""What the conflict graph under both rules (msspe_conflict_graph_dev / _edges_dev) costs beside its two screens, in one
session on one device: the thal ANY screen alone, the thal END1 screen alone, the union call, and the union call with
the ordered edge list, at the pipeline's pool size and at 8,192 random 13-mers.

    python tools/perf_conflict_graph.py [--sizes 1225,8192] [--min-seconds 1.0]

Every figure is device time between two events on the engine's stream (the caller's torch stream), read after a
synchronise, summed over as many repetitions as make up --min-seconds, after one warm-up call of the same size.
Decisions-only screens into a bitmap (and row counts), ANY threshold -9000, END threshold 10, ntthal defaults.
added_ms is what the union (and emit) kernels and the loss of the single-rule route (the two screens write planes of
the scratch a block of rows at a time, the ANY screen without its mirrored launch plan) add over the two screens' sum.
Prints one JSON line per size."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))


def packed(rng, n, k):
    codes = rng.integers(0, 4, (n, k)).astype(np.uint64)
    return (codes << (2 * np.arange(k, dtype=np.uint64))).sum(axis=1).astype(np.uint64)


def timed(torch, fn, min_seconds):
    fn()                                   # warm-up: tables, work buffers
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
    return total / reps / 1000.0          # seconds per call


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1225,8192")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    import msspe_amd

    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    chem = msspe_amd.Chem.ntthal()
    dg, tm, k = -9000.0, 10.0, 13
    both = msspe_amd.ConflictRule.of(dg, tm)
    for n in [int(x) for x in args.sizes.split(",")]:
        words = (n + 63) // 64
        d_pool = torch.from_numpy(packed(np.random.default_rng(n), n, k).view(np.int64)).cuda()
        d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_bm = torch.zeros(n * words, dtype=torch.int64, device="cuda")
        d_kinds = torch.zeros(3, dtype=torch.int64, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        sq = ((0, n), (0, n))

        def screen_any():
            eng.cross_dimer_dev(d_pool.data_ptr(), n, k, chem, dg, *sq, d_rc.data_ptr(), d_bm.data_ptr())

        def screen_end():
            eng.cross_dimer_end_dev(d_pool.data_ptr(), n, k, chem, tm, *sq, d_rc.data_ptr(), d_bm.data_ptr())

        def union():
            eng.conflict_graph_dev(d_pool.data_ptr(), n, k, chem, both, *sq, d_rc.data_ptr(), d_bm.data_ptr(),
                                   d_kinds.data_ptr())

        union()
        eng.synchronize()
        kinds = d_kinds.cpu().numpy().copy()
        cap = int(kinds.sum()) + 16
        d_edges = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")

        def union_edges():
            eng.conflict_graph_edges_dev(d_pool.data_ptr(), n, k, chem, both, *sq, d_edges.data_ptr(), cap,
                                         d_count.data_ptr(), d_rc.data_ptr(), d_bm.data_ptr(), d_kinds.data_ptr())

        t_any = timed(torch, screen_any, args.min_seconds)
        t_end = timed(torch, screen_end, args.min_seconds)
        t_union = timed(torch, union, args.min_seconds)
        t_edges = timed(torch, union_edges, args.min_seconds)
        # the ANY screen as the union runs it: a rectangle of rows, so never the mirrored launch plan
        eng.set_option("pair_mirror", 0)
        try:
            t_any_flat = timed(torch, screen_any, args.min_seconds)
        finally:
            eng.set_option("pair_mirror", "auto")
        print(json.dumps({
            "k": k, "n": n, "edges": int(kinds.sum()), "kinds": [int(x) for x in kinds],
            "any_ms": round(t_any * 1e3, 3), "any_no_mirror_ms": round(t_any_flat * 1e3, 3),
            "end_ms": round(t_end * 1e3, 3), "end_checks_per_s": round(n * n / t_end, -3),
            "union_ms": round(t_union * 1e3, 3), "union_edges_ms": round(t_edges * 1e3, 3),
            "union_added_ms": round((t_union - t_any - t_end) * 1e3, 3),
            "union_added_over_no_mirror_ms": round((t_union - t_any_flat - t_end) * 1e3, 3),
            "edges_added_ms": round((t_edges - t_union) * 1e3, 3),
            "union_added_vs_end": round((t_union - t_any - t_end) / t_end, 4),
        }), flush=True)
    eng.reset_stream()
    eng.close()


if __name__ == "__main__":
    main()
