"""Rates of the A x B screen for pools of different oligo lengths (msspe_cross_dimer_ab_dev), beside the
single-pool screen at the longer length and the dense kernel, in one session on one device.

    python tools/perf_mixed.py [--n 8192] [--dense-n 1024] [--min-seconds 1.0]

Every figure is device time between two events on the engine's stream (the caller's torch stream), read after a
synchronise, summed over as many repetitions as make up --min-seconds, after one warm-up call of the same size.
Decisions-only screens (row counts, no planes), threshold -9000, ntthal defaults.  Prints one JSON line per shape."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))

SHAPES = [(13, 20), (16, 20), (20, 24), (24, 32)]


def rand_pool(rng, n, k):
    return rng.integers(0, 4, (n, k)).astype(np.uint64)


def packed(rng, n, k):
    codes = rand_pool(rng, n, k)
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
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    import msspe_amd

    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    chem = msspe_amd.Chem.ntthal()
    rng = np.random.default_rng(1)
    n, nd = args.n, args.dense_n
    for k_a, k_b in SHAPES:
        kmax = max(k_a, k_b)
        d_a = torch.from_numpy(packed(rng, n, k_a).view(np.int64)).cuda()
        d_b = torch.from_numpy(packed(rng, n, k_b).view(np.int64)).cuda()
        d_sq = torch.from_numpy(packed(rng, n, kmax).view(np.int64)).cuda()
        d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")

        def mixed(m=n):
            eng.cross_dimer_ab_dev(d_a.data_ptr(), n, k_a, d_b.data_ptr(), n, k_b, chem, -9000.0, (0, m), (0, m),
                                   d_rc.data_ptr())

        def square():
            eng.cross_dimer_dev(d_sq.data_ptr(), n, kmax, chem, -9000.0, (0, n), (0, n), d_rc.data_ptr())

        t_mixed = timed(torch, mixed, args.min_seconds)
        eng.last_overflow_pairs()
        mixed()
        handed_on = eng.last_overflow_pairs()
        t_square = timed(torch, square, args.min_seconds)
        eng.set_option("force_generic", 1)
        try:
            t_dense = timed(torch, lambda: mixed(nd), args.min_seconds)
        finally:
            eng.set_option("force_generic", 0)
        r_mixed, r_square, r_dense = n * n / t_mixed, n * n / t_square, nd * nd / t_dense
        print(json.dumps({
            "k_a": k_a, "k_b": k_b, "n": n,
            "mixed_checks_per_s": round(r_mixed, -3),
            "equal_length_k": kmax, "equal_length_checks_per_s": round(r_square, -3),
            "dense_n": nd, "dense_checks_per_s": round(r_dense, -3),
            "mixed_vs_equal": round(r_mixed / r_square, 3), "mixed_vs_dense": round(r_mixed / r_dense, 1),
            "handed_on_frac": round(handed_on / (n * n), 5),
        }), flush=True)
    eng.reset_stream()
    eng.close()


if __name__ == "__main__":
    main()
