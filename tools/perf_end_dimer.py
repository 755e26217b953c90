"""Rates of the END screen (msspe_cross_dimer_end_dev / _end_ab_dev: thal END1 for every ordered pair) beside the thal
ANY screen on the same f64 kernels (option pair_kernel=f64) and the END screen on the dense kernel (force_generic=1),
in one session on one device.

    python tools/perf_end_dimer.py [--n 8192] [--dense-n 1024] [--big-n 65536] [--min-seconds 1.0]

Every figure is device time between two events on the engine's stream (the caller's torch stream), read after a
synchronise, summed over as many repetitions as make up --min-seconds, after one warm-up call of the same size.
Decisions-only screens (row counts, no planes), END threshold 47 (PRIMER_MAX_SELF_END_TH), ANY threshold -9000,
ntthal defaults.  Prints one JSON line per figure group; --big-n 0 skips the 65,536^2 END screen."""
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
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--dense-n", type=int, default=1024)
    ap.add_argument("--big-n", type=int, default=65536)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    import msspe_amd

    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    chem = msspe_amd.Chem.ntthal()
    rng = np.random.default_rng(1)
    n, nd = args.n, args.dense_n
    d_rc = torch.zeros(max(n, args.big_n, 1), dtype=torch.int32, device="cuda")
    for k in (13, 20):
        d_pool = torch.from_numpy(packed(rng, n, k).view(np.int64)).cuda()

        def end(m=n):
            eng.cross_dimer_end_dev(d_pool.data_ptr(), n, k, chem, 47.0, (0, m), (0, m), d_rc.data_ptr())

        def any_f64():
            eng.cross_dimer_dev(d_pool.data_ptr(), n, k, chem, -9000.0, (0, n), (0, n), d_rc.data_ptr())

        t_end = timed(torch, end, args.min_seconds)
        eng.last_overflow_pairs()
        end()
        handed_on = eng.last_overflow_pairs()
        eng.set_option("pair_kernel", "f64")
        try:
            t_any = timed(torch, any_f64, args.min_seconds)
        finally:
            eng.set_option("pair_kernel", "auto")
        eng.set_option("force_generic", 1)
        try:
            t_dense = timed(torch, lambda: end(nd), args.min_seconds)
        finally:
            eng.set_option("force_generic", 0)
        r_end, r_any, r_dense = n * n / t_end, n * n / t_any, nd * nd / t_dense
        print(json.dumps({
            "k": k, "n": n, "end_checks_per_s": round(r_end, -3),
            "any_f64_checks_per_s": round(r_any, -3), "dense_n": nd, "end_dense_checks_per_s": round(r_dense, -3),
            "end_vs_any_f64": round(r_end / r_any, 3), "end_vs_dense": round(r_end / r_dense, 1),
            "handed_on_frac": round(handed_on / (n * n), 5),
        }), flush=True)
    # A x B: 13-mers (oligo 1) against 20-mers
    d_a = torch.from_numpy(packed(rng, n, 13).view(np.int64)).cuda()
    d_b = torch.from_numpy(packed(rng, n, 20).view(np.int64)).cuda()
    t_ab = timed(torch, lambda: eng.cross_dimer_end_ab_dev(d_a.data_ptr(), n, 13, d_b.data_ptr(), n, 20, chem, 47.0,
                                                           (0, n), (0, n), d_rc.data_ptr()), args.min_seconds)
    print(json.dumps({"k_a": 13, "k_b": 20, "n": n, "end_ab_checks_per_s": round(n * n / t_ab, -3)}), flush=True)
    if args.big_n:
        nb = args.big_n
        d_big = torch.from_numpy(packed(np.random.default_rng(65536), nb, 13).view(np.int64)).cuda()
        d_rc.zero_()

        def big():
            eng.cross_dimer_end_dev(d_big.data_ptr(), nb, 13, chem, 47.0, (0, nb), (0, nb), d_rc.data_ptr())

        t_big = timed(torch, big, args.min_seconds)
        print(json.dumps({"k": 13, "n": nb, "end_checks_per_s": round(nb * nb / t_big, -3),
                          "ms_per_screen": round(t_big * 1000.0, 1)}), flush=True)
    eng.reset_stream()
    eng.close()


if __name__ == "__main__":
    main()
