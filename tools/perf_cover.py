"""Time of the device vertex cover (msspe_conflict_cover_dev, csrc/conflict_cover.hip) beside the screen that feeds it
and the host cover it replaces, per pool size, in one session on one device.

    python tools/perf_cover.py [--sizes 2000,16384,65536] [--host-max 16384] [--reps 3]

Pools: msspe_amd.synth.random_pool(n, 13) with bench.py's seed (the 65,536 pool is the headline screen's), duplicate
13-mers removed (the graph's nodes are distinct).  Screen: msspe_cross_dimer_dev, decisions only (bitmap), -9000,
ntthal defaults, device time between two events after one warm-up call.  Cover: the call's own phase times (device
events inside the call: sort and keys, S = B | B^T, rounds -- the rounds include the host's reads of the done word once
per 16 rounds) and its wall time, after one warm-up call; the mean of --reps calls.  Host: odm_vertex_cover (the host
library's vertex_cover on the edge list as text, what the CLI's default path runs) for pools up to --host-max, and the
time to build that text from msspe_cross_dimer_edges.  One JSON line per size."""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--host-max", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import msspe_amd

    eng = msspe_amd.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    chem = msspe_amd.Chem.ntthal()
    host = C.CDLL(str(ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"))
    for n0 in (int(s) for s in args.sizes.split(",")):
        words = list(dict.fromkeys(msspe_amd.synth.pool_strings(msspe_amd.synth.random_pool(n0, 13))))
        n = len(words)
        wds = (n + 63) // 64
        d_pool = torch.from_numpy(msspe_amd.pack_oligos(words).view(np.int64)).cuda()
        d_bm = torch.zeros((n, wds), dtype=torch.int64, device="cuda")
        d_del = torch.zeros(n, dtype=torch.uint8, device="cuda")

        def screen():
            eng.cross_dimer_dev(d_pool.data_ptr(), n, 13, chem, -9000.0, (0, n), (0, n), d_bitmap=d_bm.data_ptr())

        screen()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        screen()
        e1.record()
        torch.cuda.synchronize()
        screen_ms = e0.elapsed_time(e1)
        lut = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)
        bm = d_bm.cpu().numpy().view(np.uint8)
        edges_ordered = int(sum(lut[bm[r:r + 4096]].sum() for r in range(0, n, 4096)))

        n_del = eng.conflict_cover_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_del.data_ptr())   # warm-up
        wall, ph = [], np.zeros(3)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            nd = eng.conflict_cover_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_del.data_ptr())
            wall.append((time.perf_counter() - t0) * 1000.0)
            assert nd == n_del
            ph += [eng.info("cover_keys_us"), eng.info("cover_symmetrise_us"), eng.info("cover_rounds_us")]
        ph /= args.reps
        rounds = eng.info("cover_rounds")
        out = {"n": n, "pool_rows": n0, "conflicting_ordered_pairs": edges_ordered, "deleted": n_del,
               "screen_ms": round(screen_ms, 3), "cover_wall_ms": round(float(np.mean(wall)), 3),
               "keys_ms": round(ph[0] / 1000.0, 3), "symmetrise_ms": round(ph[1] / 1000.0, 3),
               "rounds_ms": round(ph[2] / 1000.0, 3), "rounds": rounds,
               "per_round_us": round(ph[2] / max(rounds, 1), 2)}
        if n <= args.host_max:
            t0 = time.perf_counter()
            es, cnt = eng.cross_dimer_edges(words, chem, -9000.0, capacity=max(1 << 20, 2 * edges_ordered))
            text = "\n".join(f"{words[a]},{words[b]}" for a, b in zip(es["a"].tolist(), es["b"].tolist())).encode()
            prim = "\n".join(words).encode()
            t1 = time.perf_counter()
            buf = C.create_string_buffer(16 * n + 64)
            rc = host.odm_vertex_cover(prim, text, buf, 16 * n + 64)
            t2 = time.perf_counter()
            assert rc >= 0
            got = set(buf.value.decode().split())
            dev = d_del.cpu().numpy().astype(bool)
            assert got == {w for w, d in zip(words, dev) if d}, "device and host covers differ"
            out.update({"host_edge_text_ms": round((t1 - t0) * 1000.0, 1), "host_cover_ms": round((t2 - t1) * 1000.0, 1)})
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
