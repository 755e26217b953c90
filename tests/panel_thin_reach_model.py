"""Brute-force numpy restatement of msspe_panel_thin_reach* (include/msspe_hip.h), written from its semantics on top of
the reach model (tests/stream_reach_model.py), the site model (tests/background_model.py) and the scored-site model
(tests/background_thal_model.py): one boolean array per primer over the stream.

R_p is the union, over the stable sites of primer p alone, of [pos, min(pos + D, e_r) - 1] for a plus site and
[max(pos + k - D, s_r), pos + k - 1] for a minus site, r the site's record.  C starts as the union of the forced
primers' sets; a round picks the unforced, unpicked p with the greatest |R_p \\ C| (ties: the lowest index), stops when
that gain is below min_gain, and otherwise sets C |= R_p.  The kept panel's records are the reach model's over the kept
primers' sites.  Also renders the block od-msspe-hip --thin-reach prints before "Target reach"."""
from __future__ import annotations

import numpy as np

import background_model as bm
import background_thal_model as btm
import stream_reach_model as srm


def primer_columns(k: int, sites, records, D: int, n: int, starts=None) -> np.ndarray:
    """bool (n, total_len): row p is R_p.  sites: records with the fields primer, pos and strand, all taken as stable."""
    assert D >= k
    own_starts, total = bm.record_starts(records)
    if starts is None:
        starts = own_starts
    lens = [len(r) for r in records]
    R = np.zeros((n, int(total)), dtype=bool)
    bounds = [(int(s), int(s) + ln) for s, ln in zip(np.asarray(starts).astype(np.int64).tolist(), lens)]
    for site in np.asarray(sites):
        p, pos, minus = int(site["primer"]), int(site["pos"]), int(site["strand"])
        s, e = next((s, e) for s, e in bounds if s <= pos and pos + k <= e)
        if minus:
            R[p, max(pos + k - D, s):pos + k] = True
        else:
            R[p, pos:min(pos + D, e)] = True
    return R


def greedy(R: np.ndarray, min_gain: int = 1, forced=None):
    """(keep uint8[n], order, gains, covered bool[total]) of the rule above."""
    n = R.shape[0]
    keep = np.zeros(n, dtype=np.uint8)
    if forced is not None:
        keep[:] = np.asarray(forced) != 0
    covered = R[keep != 0].any(axis=0) if n else np.zeros(R.shape[1], dtype=bool)
    live = keep == 0
    order, gains = [], []
    while live.any():
        gain = (R & ~covered).sum(axis=1)
        gain[~live] = -1
        p = int(np.argmax(gain))                       # the first of equals: the lowest index
        if gain[p] < min_gain:
            break
        order.append(p)
        gains.append(int(gain[p]))
        covered = covered | R[p]
        live[p] = False
        keep[p] = 1
    return keep, np.array(order, dtype=np.uint32), np.array(gains, dtype=np.uint32), covered


def thin_of_sites(k: int, sites, records, n: int, D: int, min_gain: int = 1, forced=None, starts=None) -> dict:
    """Everything the call returns but the site counts, from a site list whose every entry is stable."""
    sites = np.asarray(sites)
    R = primer_columns(k, sites, records, D, n, starts)
    keep, order, gains, covered = greedy(R, min_gain, forced)
    kept_sites = sites[keep[sites["primer"].astype(np.int64)] != 0] if len(sites) else sites
    return {"keep": keep, "order": order, "gains": gains, "primer_reach": R.sum(axis=1).astype(np.uint32),
            "reached_all": int(R.any(axis=0).sum()) if n else 0, "reached_kept": int(covered.sum()),
            "records": srm.reach_of_sites(k, kept_sites, records, D, starts)}


def thin(tables, records, primers, M: int, E: int, mode, tm_threshold: float, D: int, min_gain: int = 1, forced=None,
         args=None, scored=None) -> dict:
    """The whole call: thin_of_sites' dict plus counts and stable (n, 2) of the whole panel.  tm_threshold <= 0: every
    site of the string rule is stable and no thal is needed (tables may be None)."""
    primers = list(primers)
    k = len(primers[0]) if primers else 0
    if tm_threshold <= 0 and scored is None:
        counts, sites = bm.sites(records, primers, M, E)
        stable = counts
    else:
        counts, stable, recs = scored if scored is not None else btm.scored_sites(tables, records, primers, M, E, mode,
                                                                                  tm_threshold, args)
        sites = recs[recs["stable"] != 0]
    out = thin_of_sites(k, sites, records, len(primers), D, min_gain, forced)
    out["counts"], out["stable"] = counts, stable
    return out


def render(res: dict, D: int, min_gain: int, M: int, E: int, mode=None, tm_threshold=None, forced=None) -> str:
    """The block od-msspe-hip --thin-reach prints before "Target reach"."""
    n = len(res["keep"])
    n_forced = int((np.asarray(forced) != 0).sum()) if forced is not None else 0
    out = (f"\nReach thinning (extension {D} bases, min gain {min_gain}; sites: "
           f"{srm.rule_text(M, E, mode, tm_threshold)}):\n")
    out += f"  Kept {int(res['keep'].sum())} of {n} primers ({n_forced} forced)\n"
    out += f"  Columns reached by all: {res['reached_all']}, by kept: {res['reached_kept']}\n"
    return out
