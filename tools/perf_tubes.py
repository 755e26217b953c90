"""Time of the tube split (msspe_conflict_tubes_dev, csrc/tube_split.hip) beside the device vertex cover on the same
bitmap, per pool size, in one session on one device.

    python tools/perf_tubes.py [--sizes 2000,16384,65536] [--tubes 64,8] [--reps 3]

Pools: msspe_amd.synth.random_pool(n, 13) with bench.py's seed, duplicate 13-mers removed (2,000, 16,383 and 65,503
distinct oligos).  Screen: msspe_cross_dimer_dev, decisions only (bitmap), -9000, ntthal defaults, once per pool.  Tube
split, per value of --tubes: the call's own phase times (device events inside the call: sort and keys, S = B | B^T, the
keys, waits and rounds -- the rounds include the host's reads of the done word once per 16 rounds) and its wall time,
after one warm-up call; the mean of --reps calls; rounds, tubes used, unplaced.  Cover: msspe_conflict_cover_dev on the
same bitmap, measured the same way.  One JSON line per size."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,16384,65536")
    ap.add_argument("--tubes", default="64,8")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import msspe_amd

    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    chem = msspe_amd.Chem.ntthal()
    for n0 in (int(s) for s in args.sizes.split(",")):
        words = list(dict.fromkeys(msspe_amd.synth.pool_strings(msspe_amd.synth.random_pool(n0, 13))))
        n = len(words)
        wds = (n + 63) // 64
        d_pool = torch.from_numpy(msspe_amd.pack_oligos(words).view(np.int64)).cuda()
        d_bm = torch.zeros((n, wds), dtype=torch.int64, device="cuda")
        d_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        eng.cross_dimer_dev(d_pool.data_ptr(), n, 13, chem, -9000.0, (0, n), (0, n), d_bitmap=d_bm.data_ptr())
        torch.cuda.synchronize()
        out = {"n": n, "pool_rows": n0}

        def timed(call, keys):
            first = call()                                   # warm-up
            wall, ph = [], np.zeros(3)
            for _ in range(args.reps):
                t0 = time.perf_counter()
                assert call() == first
                wall.append((time.perf_counter() - t0) * 1000.0)
                ph += [eng.info(k) for k in keys]
            ph /= args.reps
            return first, {"wall_ms": round(float(np.mean(wall)), 3), "keys_ms": round(ph[0] / 1000.0, 3),
                           "symmetrise_ms": round(ph[1] / 1000.0, 3), "rounds_ms": round(ph[2] / 1000.0, 3)}

        for t in (int(x) for x in args.tubes.split(",")):
            (used, unplaced), rec = timed(
                lambda: eng.conflict_tubes_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_out.data_ptr(), t),
                ("tube_keys_us", "tube_symmetrise_us", "tube_rounds_us"))
            rec.update({"rounds": eng.info("tube_rounds"), "tubes_used": used, "unplaced": unplaced})
            out[f"tubes_{t}"] = rec
        deleted, rec = timed(lambda: eng.conflict_cover_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_out.data_ptr()),
                             ("cover_keys_us", "cover_symmetrise_us", "cover_rounds_us"))
        rec.update({"rounds": eng.info("cover_rounds"), "deleted": deleted})
        out["cover"] = rec
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
