"""Brute-force numpy restatement of msspe_stream_reach* (include/msspe_hip.h), written from its semantics on top of the
site model (tests/background_model.py) and the scored-site model (tests/background_thal_model.py): one boolean array
per record.

Record r spans the stream columns [s_r, e_r).  P_r / M_r: the positions of its stable plus- / minus-strand sites (any
primer; several primers at one position count once).  With reach D, column b of r is plus-reached iff some p in P_r
has p <= b <= p + D - 1, minus-reached iff some q in M_r has q + k - D <= b <= q + k - 1; reach never leaves the
record, and invalid columns are columns like any other.  Per record: |P_r|, |M_r|, the plus / minus / either / both
reached columns and, per strand and for "neither", the longest maximal run of unreached columns (ties: the lowest
position; length 0: position s_r).  Also renders the block od-msspe-hip --reach prints and the --reach-out CSV."""
from __future__ import annotations

import numpy as np

import background_model as bm
import background_thal_model as btm

REACH_RECORD_DTYPE = np.dtype([(f, np.uint32) for f in (
    "sites_plus", "sites_minus", "reached_plus", "reached_minus", "reached_either", "reached_both",
    "gap_plus_len", "gap_plus_pos", "gap_minus_len", "gap_minus_pos", "gap_either_len", "gap_either_pos")])
FIELDS = REACH_RECORD_DTYPE.names


def longest_false_run(reached: np.ndarray) -> tuple[int, int]:
    """(length, offset) of the longest maximal run of False; the lowest offset among equals; (0, 0) without one."""
    edge = np.diff(np.concatenate(([True], np.asarray(reached, dtype=bool), [True])).astype(np.int8))
    first, behind = np.flatnonzero(edge == -1), np.flatnonzero(edge == 1)      # run i is [first[i], behind[i])
    if not len(first):
        return 0, 0
    i = int(np.argmax(behind - first))                                         # the first of equals
    return int(behind[i] - first[i]), int(first[i])


def reach_of_sites(k: int, sites, records, D: int, starts=None) -> np.ndarray:
    """sites: records with the fields pos and strand (SITE_DTYPE or SCORED_SITE_DTYPE), every one taken as stable.
    starts: the record starts when they are not those of `records` as a stream (a stream taken as ONE record:
    records = [the stream's text], starts = None)."""
    assert D >= k
    if starts is None:
        starts, _total = bm.record_starts(records)
    lens = [len(r) for r in records]
    sites = np.asarray(sites)
    pos, strand = sites["pos"].astype(np.int64), sites["strand"]
    out = np.zeros(len(records), dtype=REACH_RECORD_DTYPE)
    for r, (s, n) in enumerate(zip(np.asarray(starts).astype(np.int64).tolist(), lens)):
        e = s + n
        inside = (pos >= s) & (pos + k <= e)
        P = np.unique(pos[inside & (strand == 0)])
        M = np.unique(pos[inside & (strand == 1)])
        plus = np.zeros(n, dtype=bool)
        minus = np.zeros(n, dtype=bool)
        for p in P.tolist():
            plus[p - s:min(p + D, e) - s] = True
        for q in M.tolist():
            minus[max(q + k - D, s) - s:q + k - s] = True
        rec = out[r]
        rec["sites_plus"], rec["sites_minus"] = len(P), len(M)
        rec["reached_plus"], rec["reached_minus"] = int(plus.sum()), int(minus.sum())
        rec["reached_either"], rec["reached_both"] = int((plus | minus).sum()), int((plus & minus).sum())
        for name, arr in (("plus", plus), ("minus", minus), ("either", plus | minus)):
            length, at = longest_false_run(arr)
            rec[f"gap_{name}_len"], rec[f"gap_{name}_pos"] = length, s + at
    return out


def reach_of_scored(k: int, scored, records, D: int, starts=None) -> np.ndarray:
    """The same from the scored-site model's records (SCORED_SITE_DTYPE): the stable ones reach."""
    return reach_of_sites(k, scored[scored["stable"] != 0], records, D, starts)


def reach(tables, records, primers, M: int, E: int, mode, tm_threshold: float, D: int, args=None, scored=None):
    """(site counts, stable counts, REACH_RECORD_DTYPE array).  tm_threshold <= 0: every site of the string rule is
    stable and no thal is needed (tables may be None)."""
    primers = list(primers)
    k = len(primers[0]) if primers else 0
    if tm_threshold <= 0 and scored is None:
        counts, sites = bm.sites(records, primers, M, E)
        return counts, counts, reach_of_sites(k, sites, records, D)
    counts, stable, recs = scored if scored is not None else btm.scored_sites(tables, records, primers, M, E, mode,
                                                                              tm_threshold, args)
    return counts, stable, reach_of_scored(k, recs, records, D)


def rule_text(M: int, E: int, mode=None, tm_threshold=None) -> str:
    out = f"up to {M} mismatches, last {E} bases exact"
    if tm_threshold is not None:
        name = {1: "ANY", 2: "END1", "any": "ANY", "end1": "END1"}[mode]
        out += "; stable: thal %s t >= %.2f C" % (name, float(np.float32(tm_threshold)))
    return out


def render(names, records, recs, D: int, M: int, E: int, mode=None, tm_threshold=None) -> str:
    """The block od-msspe-hip --reach prints last; names: the genomes' names, records: their ungapped rows."""
    starts, _total = bm.record_starts(records)
    starts = starts.astype(np.int64)
    r = {f: recs[f].astype(np.int64) for f in FIELDS}
    out = f"\nTarget reach (extension {D} bases; sites: {rule_text(M, E, mode, tm_threshold)}):\n"
    out += (f"  Total: {len(records)} genomes, {sum(len(x) for x in records)} columns, reached plus "
            f"{int(r['reached_plus'].sum())}, minus {int(r['reached_minus'].sum())}, either "
            f"{int(r['reached_either'].sum())}, both {int(r['reached_both'].sum())}\n")
    out += f"  Genomes with a gap above {D}: {int((r['gap_either_len'] > D).sum())}\n"
    order = sorted(range(len(records)), key=lambda i: (-int(r["gap_either_len"][i]), i))[:20]
    out += f"  Longest gaps, {len(order)} genomes (name: offset, length):\n"
    for i in order:
        out += f"    {names[i]}: {int(r['gap_either_pos'][i] - starts[i])}, {int(r['gap_either_len'][i])}\n"
    return out


def render_csv(names, records, recs) -> str:
    """--reach-out: one line per genome with every field, positions as offsets in the ungapped genome."""
    starts, _total = bm.record_starts(records)
    out = "name,columns," + ",".join(FIELDS) + "\n"
    for i, nm in enumerate(names):
        vals = [int(recs[f][i]) - (int(starts[i]) if f.endswith("_pos") else 0) for f in FIELDS]
        out += f"{nm},{len(records[i])}," + ",".join(map(str, vals)) + "\n"
    return out
