"""Device time of coverage within N mismatches (msspe_segment_coverage_mm_packed_dev) beside the exact call
(msspe_segment_coverage_packed_dev) at config2 size: msspe_amd.synth.aligned_genomes(10000, 30000) resident in packed
form, the fixture's kept panel (tests/golden/config2_10k.json), segment 500 / stride 250 / window 50, in one session on
one device.

    python tools/perf_coverage_mm.py [--rows 10000] [--length 30000] [--min-seconds 1.0] [--cpu-sample 200]

Every figure is device time between two events on the engine's stream, read after a synchronise, summed over as many
repetitions as make up --min-seconds, after one warm-up call (the calls copy best -- and the counts -- back to the host
and synchronise, so that copy is inside the figure).  Comparisons = valid-or-not window positions x primers of their
direction.  VALU per comparison is read from the kernel's ISA; the issue bound is 256 CUs x 128 lanes per
clock x 2.4 GHz.  The CPU line is a 16-thread numpy restatement (tests/coverage_mm_model.py) on --cpu-sample segments,
scaled to all segments: labelled as such, it is not a measurement of the whole alignment.
Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))
sys.path.insert(0, str(ROOT / "tests"))

VALU_PER_CMP = 5.656          # both word widths, the inner loop of k_coverage_mm<.., false>
ISSUE_BOUND = 256 * 128 * 2.4e9


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
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--cpu-sample", type=int, default=200)
    args = ap.parse_args()
    import torch
    import msspe_amd

    fx = json.loads((ROOT / "tests" / "golden" / "config2_10k.json").read_text())
    fwd13, rev13 = fx["primers_kept"]["F"], fx["primers_kept"]["R"]
    g = msspe_amd.synth.aligned_genomes(args.rows, args.length)
    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    hp = eng.put_rows_packed(g)
    n, L = g.shape
    seg, stride, W = 500, 250, 50
    P = (L - seg) // stride + 1
    rng = np.random.default_rng(24)
    # a k = 24 panel of the same size: windows of the alignment's first row (no gap or N in them)
    row = bytes(g[0]).decode()
    starts = [c for c in rng.integers(0, L - 24, 4 * len(fwd13)) if set(row[c:c + 24]) <= set("ACGT")]
    fwd24 = [row[c:c + 24] for c in starts[:len(fwd13)]]
    rev24 = [row[c:c + 24] for c in starts[len(fwd13):len(fwd13) + len(rev13)]]
    try:
        cases = [("exact", 13, None, None, False)]
        cases += [("mm", 13, M, 3, cnt) for M in (1, 2) for cnt in (False, True)]
        cases += [("mm", 24, 2, 3, False)]
        t_exact = None
        for kind, k, M, E, cnt in cases:
            opt = msspe_amd.KmerOpt(seg, stride, W, k, 0, 0)
            f, r = (fwd13, rev13) if k == 13 else (fwd24, rev24)
            if kind == "exact":
                d_f = msspe_amd.pack_oligos(f)
                d_r = msspe_amd.pack_oligos(r)
                hit = np.zeros(n * P, dtype=np.uint8)
                import ctypes as C

                def fn():
                    eng._check(eng.L.msspe_segment_coverage_packed_dev(
                        eng.ptr, C.c_void_p(hp), n, L, C.byref(opt), d_f.ctypes.data, len(d_f), d_r.ctypes.data,
                        len(d_r), hit.ctypes.data))
            else:
                fn = (lambda opt=opt, f=f, r=r, M=M, E=E, cnt=cnt:
                      eng.segment_coverage_mm_packed(hp, n, L, opt, f, r, M, E, per_primer=cnt))
            t = timed(torch, fn, args.min_seconds)
            comps = n * P * (W - k + 1) * (len(f) + len(r))
            line = {"case": kind, "k": k, "n_fwd": len(f), "n_rev": len(r), "segments": n * P, "ms": round(t * 1e3, 3)}
            if kind == "exact":
                t_exact = t
            else:
                rate = comps / t
                line.update({"M": M, "E": E, "counts": cnt, "comparisons": comps,
                             "comparisons_per_s": float("%.4g" % rate), "valu_per_comparison": VALU_PER_CMP,
                             "issue_bound_frac": round(rate * VALU_PER_CMP / ISSUE_BOUND, 3),
                             "vs_exact": round(t / t_exact, 2)})
            print(json.dumps(line), flush=True)
    finally:
        eng.device_free(hp)
        eng.reset_stream()
        eng.close()
    # CPU figure: the numpy model, 16 threads, on a sample of segments, scaled to all of them
    import coverage_mm_model as cm
    pick = rng.choice(n * P, size=args.cpu_sample, replace=False)
    segs = [(int(i // P), int(i % P)) for i in pick]
    parts = [segs[i::16] for i in range(16)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda s: cm.best_and_counts(g, seg, stride, W, 13, fwd13, rev13, 2, 3, segments=s, chunk=4), parts))
    t_cpu = time.perf_counter() - t0
    print(json.dumps({"case": "cpu_numpy_16_threads_scaled", "k": 13, "M": 2, "E": 3, "sample_segments": args.cpu_sample,
                      "sample_s": round(t_cpu, 3), "scaled_s_all_segments": round(t_cpu * n * P / args.cpu_sample, 1)}),
          flush=True)


if __name__ == "__main__":
    main()
