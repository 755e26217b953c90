"""Restatement of msspe_background_thal* (include/msspe_hip.h), written from its semantics on top of the site model
(tests/background_model.py) and the CPU oracle's thal (oracle/pyoracle.py).

A site {primer u, pos p, strand s} of the background screen, w the k columns at p: the TEMPLATE OLIGO o2 is the strand
the primer anneals to, 5'->3': revcomp(w) on the plus strand (0), w itself on the minus strand (1).  The site score is
thal(u, o2), mode 1 ANY or 2 END1; raw dG is +inf and raw t is 0 without a structure.  t_site = max(0, t); the site is
STABLE iff not (round_fixed_f32(t_site, 2) < float32(tm_threshold)).  Also renders the block od-msspe-hip prints with
--background-tm."""
from __future__ import annotations

import numpy as np

import background_model as bm
import pyoracle

SCORED_SITE_DTYPE = np.dtype([("primer", np.uint32), ("pos", np.uint32), ("mismatches", np.uint16),
                              ("strand", np.uint16), ("stable", np.uint32), ("dg", np.float64), ("t", np.float64)])
MODES = {"any": pyoracle.ANY, "end1": pyoracle.END1}


def stream_text(records) -> str:
    return "-".join(r if isinstance(r, str) else bytes(r).decode("latin-1") for r in records)


def template_oligo(stream: str, k: int, pos: int, strand: int) -> str:
    w = stream[pos:pos + k]
    return w if strand else bm.revcomp(w)


def template_oligos(records, primers, sites) -> list[str]:
    k = len(primers[0]) if len(primers) else 0
    s = stream_text(records)
    return [template_oligo(s, k, int(r["pos"]), int(r["strand"])) for r in sites]


def is_stable(t: float, tm_threshold: float) -> bool:
    t_site = t if t > 0.0 else 0.0
    return not (pyoracle.round_fixed_f32(t_site, 2) < float(np.float32(tm_threshold)))


def score(tables, primers, sites, o2, mode, args=None):
    """(dg, t) float64 arrays: the oracle's raw doubles of every site."""
    mode = MODES[mode] if isinstance(mode, str) else mode
    dg = np.empty(len(sites))
    t = np.empty(len(sites))
    cache = {}
    for i, (r, b) in enumerate(zip(sites, o2)):
        key = (primers[int(r["primer"])], b)
        if key not in cache:
            res = pyoracle.thal(tables, key[0], key[1], mode, args)
            cache[key] = (np.inf, 0.0) if res.no_structure else (res.dG, res.t)
        dg[i], t[i] = cache[key]
    return dg, t


def records_of(sites, dg, t, tm_threshold) -> np.ndarray:
    out = np.zeros(len(sites), dtype=SCORED_SITE_DTYPE)
    for f in bm.SITE_DTYPE.names:
        out[f] = sites[f]
    out["dg"], out["t"] = dg, t
    out["stable"] = [is_stable(float(x), tm_threshold) for x in t]
    return out


def stable_counts(n: int, recs) -> np.ndarray:
    counts = np.zeros((n, 2), dtype=np.uint64)
    keep = recs[recs["stable"] != 0]
    np.add.at(counts, (keep["primer"].astype(np.int64), keep["strand"].astype(np.int64)), 1)
    return counts


def scored_sites(tables, records, primers, M: int, E: int, mode, tm_threshold: float, args=None):
    """(counts (n, 2), stable (n, 2), records sorted by (primer, strand, pos))."""
    primers = list(primers)
    counts, sites = bm.sites(records, primers, M, E)
    o2 = template_oligos(records, primers, sites)
    dg, t = score(tables, primers, sites, o2, mode, args)
    recs = records_of(sites, dg, t, tm_threshold)
    return counts, stable_counts(len(primers), recs), recs


def render(names, counts, stable, M: int, E: int, mode, tm_threshold: float) -> str:
    """The block od-msspe-hip --background ... --background-tm prints after the coverage report."""
    name = {1: "ANY", 2: "END1", "any": "ANY", "end1": "END1"}[mode]
    thr = "%.2f" % float(np.float32(tm_threshold))
    out = f"\nBackground sites (up to {M} mismatches, last {E} bases exact; stable: thal {name} t >= {thr} C):\n"
    c = np.asarray(counts, dtype=np.uint64).reshape(-1, 2)
    s = np.asarray(stable, dtype=np.uint64).reshape(-1, 2)
    for nm, (plus, minus), (sp, sm) in zip(names, c.tolist(), s.tolist()):
        out += f"  {nm}: plus {plus}, minus {minus}, stable plus {sp}, minus {sm}\n"
    out += (f"  Total: {len(c)} primers, plus {int(c[:, 0].sum())}, minus {int(c[:, 1].sum())}, "
            f"stable plus {int(s[:, 0].sum())}, minus {int(s[:, 1].sum())}\n")
    return out
