#!/usr/bin/env python3
"""Writes tests/golden/headline_65536.json: bench.py's headline screen (65,536 random 13-mers, every ordered pair
through thal ANY at the default ntthal chemistry, threshold -9000) decided by the CPU oracle on about 2,340 whole rows.
Run once on a CPU machine (no GPU; about 12 minutes on 8 cores, a few MB of memory):

    python tools/make_headline_fixture.py [--out tests/golden/headline_65536.json] [--block 64] [--threads 0]

The rows are chosen where the row kernel's 65,536^2 call can go wrong without the small pools noticing:
  G  group_rows(65536, 32, 0): eight 256-row groups spread over the whole range, half of them at or above
     32,768 (block offsets past 2^31 pairs); a subset of rank 0 of 8 under the dealt-rows rule;
  B  16 rows on each side of every launch boundary of the 65,536-row call (csrc/screen_plan.hpp splits a block into
     launches of at most kChunkPairs pairs, in whole 24-row groups: launch_boundaries below asks the library);
  T  the last 32 rows.
Every row is screened against all 65,536 columns.  Per row the fixture keeps the conflict count and an 8-byte
BLAKE2b digest of the row's decisions packed little-endian into bytes: the same bytes as row r of the engine's
conflict bitmap (bm[r].view(np.uint8)), since 65,536 is a multiple of 64.  The row sets are stored as [r0, r1)
ranges, `rows` / `counts` / `digests` as aligned lists; a regeneration differs only in wall_time_s.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))
sys.path.insert(0, str(ROOT / "oracle"))

N, K, THRESHOLD = 65536, 13, -9000.0
BAND, TAIL = 16, 32


def launch_boundaries(n_rows: int, ncols: int) -> list[int]:
    """First rows (block-relative) of the second and later launches of a decisions-only call over n_rows x ncols: the
    engine's own plan for lists of 2^30 entries, which a screen of this size gets (host code, no GPU)."""
    from msspe_amd import capi
    return capi.host_screen_plan("row", 0, n_rows, 0, ncols, 1 << 30)[1:, 0].tolist()


def row_sets(n: int = N) -> dict[str, list[int]]:
    from msspe_amd import group_rows
    bands = sorted({r for b in launch_boundaries(n, n) for r in range(b - BAND, b + BAND) if 0 <= r < n})
    return {"G": [int(r) for r in group_rows(n, 32, 0)], "B": bands, "T": list(range(n - TAIL, n))}


def row_digest(cf_row: np.ndarray) -> str:
    """8-byte BLAKE2b of one row's decisions (uint8 0/1 per column), packed as the engine's bitmap row."""
    return hashlib.blake2b(np.packbits(cf_row, bitorder="little").tobytes(), digest_size=8).hexdigest()


def pool_sha256(pool: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(pool, dtype=np.uint8).tobytes()).hexdigest()


def runs(rows: list[int], block: int):
    """Contiguous [r0, r1) ranges of at most `block` rows covering the sorted, unique `rows`."""
    i = 0
    while i < len(rows):
        j = i + 1
        while j < len(rows) and rows[j] == rows[j - 1] + 1 and j - i < block:
            j += 1
        yield rows[i], rows[j - 1] + 1
        i = j


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "headline_65536.json"))
    ap.add_argument("--block", type=int, default=64, help="rows per oracle call")
    ap.add_argument("--threads", type=int, default=0, help="oracle threads (0: OpenMP's default)")
    ap.add_argument("--max-rows", type=int, default=0, help="stop after this many rows (timing a trial; no file)")
    a = ap.parse_args()

    import pyoracle
    from msspe_amd import synth

    pool = synth.random_pool(N, K)
    sets = row_sets(N)
    rows = sorted(set().union(*map(set, sets.values())))
    tables = pyoracle.Tables()
    args = pyoracle.ntthal_args()
    counts, digests = {}, {}
    t0 = time.time()
    for r0, r1 in runs(rows, a.block):
        _, _, cf, _ = pyoracle.pool_pairs(tables, pool, args, THRESHOLD, pyoracle.ANY, rows=(r0, r1),
                                          threads=a.threads, want_dg=False)
        for i, r in enumerate(range(r0, r1)):
            counts[r] = int(cf[i].sum())
            digests[r] = row_digest(cf[i])
        done = len(counts)
        el = time.time() - t0
        print(f"rows [{r0}, {r1}): {done}/{len(rows)} done, {el:.0f} s, "
              f"{done * N / el:.3g} checks/s, ~{el * (len(rows) - done) / done:.0f} s left", flush=True)
        if a.max_rows and done >= a.max_rows:
            return
    wall = time.time() - t0
    chem = {f: getattr(args, f) for f, _ in pyoracle.ThalArgs._fields_}
    chem["temp_c"] = round(chem.pop("temp_k") - 273.15, 6)
    doc = {
        "provenance": "tools/make_headline_fixture.py: oracle/pyoracle.pool_pairs (want_dg=False) on whole rows "
                      "of bench.py's headline pool",
        "command": "python tools/make_headline_fixture.py",
        "pool": {"generator": "msspe_amd.synth.random_pool", "n": N, "k": K, "seed": synth.POOL_SEED,
                 "sha256": pool_sha256(pool)},
        "k": K,
        "chem": chem,
        "threshold": THRESHOLD,
        "mode": "ANY",
        "digest": "blake2b(np.packbits(conflict_row, bitorder='little').tobytes(), digest_size=8).hexdigest()",
        "launch_boundaries": launch_boundaries(N, N),
        "row_sets": {name: [list(r) for r in runs(v, len(v))] for name, v in sets.items()},   # [r0, r1) ranges
        "rows": rows,
        "counts": [counts[r] for r in rows],
        "digests": [digests[r] for r in rows],
        "wall_time_s": round(wall, 1),
    }
    # one key per line, lists on a single line: small, and a regeneration diffs as a few changed lines
    text = "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}"
                              for k, v in doc.items()) + "\n}\n"
    Path(a.out).write_text(text)
    print(f"wrote {a.out}: {len(rows)} rows, {sum(counts.values())} conflicts, {wall:.0f} s", flush=True)


if __name__ == "__main__":
    main()
