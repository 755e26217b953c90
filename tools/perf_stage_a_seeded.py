#!/usr/bin/env python3
"""GPU timing of seeded stage A at BASELINE configs[2]'s shape (10,000 x 30,000, packed once): per direction the
unseeded call and calls seeded with the first 100 and 500 winners (max_iterations - m: they must return the rest of
the winners, which is checked).  Event-timed on the device around each blocking call; best of `reps`.  For the
seeding kernel's share run it under `rocprofv3 --kernel-trace --stats` (k_seed against the stage's other kernels).

usage: tools/perf_stage_a_seeded.py [rows] [length] [reps]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))
import torch
import msspe_amd as m

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
length = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
g = m.synth.aligned_genomes(rows, length)
eng = m.Engine(0)
d = eng.put_rows_packed(g)
mm = max(1, min(10, -(-rows // 50)))


def timed(opt, direction, seed=None):
    best, out = None, None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = eng.kmer_candidates_packed(d, rows, length, opt, direction, seed=seed)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best, out


results = []
for direction in (0, 1):
    base_ms, (w, f) = timed(m.KmerOpt(500, 250, 50, 13, 1000, mm), direction)
    line = {"direction": direction, "winners": len(w), "unseeded_ms": round(base_ms, 3)}
    for n_seed in (100, 500):
        if n_seed >= len(w):
            continue
        ms, (w2, f2) = timed(m.KmerOpt(500, 250, 50, 13, 1000 - n_seed, mm), direction, seed=w[:n_seed])
        assert w2 == w[n_seed:] and f2.tolist() == f[n_seed:].tolist(), f"prefix invariant broken at {n_seed}"
        line[f"seeded_{n_seed}_ms"] = round(ms, 3)
    results.append(line)
    print(json.dumps(line), flush=True)
eng.device_free(d)
eng.close()
