"""numpy restatement of msspe_background_amplicons* (include/msspe_hip.h), written from its semantics on top of the
scored-site model (tests/background_thal_model.py): the stable records of that model, paired by brute force.

An AMPLICON is an ordered pair of stable sites, a plus-strand site of primer fwd at stream position p and a minus-strand
site of primer rev at q, with q >= p, min_len <= len = q + k - p <= max_len, and both windows in one record:
start[r] <= p and q + k <= start[r] + len(record r).  fwd == rev and q == p are allowed; duplicate primers count
independently; every qualifying (plus site, minus site) pair is one amplicon.  Also renders the block od-msspe-hip
prints with --background-amplicon-max."""
from __future__ import annotations

import numpy as np

import background_model as bm
import background_thal_model as btm

AMPLICON_DTYPE = np.dtype([("fwd", np.uint32), ("rev", np.uint32), ("pos", np.uint32), ("len", np.uint32)])


def pair_sites(n: int, k: int, sites, records, min_len: int, max_len: int):
    """sites: records with the fields primer, pos, strand (SITE_DTYPE or SCORED_SITE_DTYPE), every one of them taken as
    stable.  Every plus site is held against every minus site (in blocks of plus sites, to bound the memory).
    Returns (counts uint64 (n, 2): amplicons as forward / as reverse, total, list sorted by (pos, len, fwd, rev))."""
    starts, _total = bm.record_starts(records)
    starts = starts.astype(np.int64)
    ends = starts + np.array([len(r) for r in records], dtype=np.int64)
    sites = np.asarray(sites)
    plus, minus = sites[sites["strand"] == 0], sites[sites["strand"] == 1]
    p, q = plus["pos"].astype(np.int64), minus["pos"].astype(np.int64)
    out = []
    if len(p) and len(q) and len(starts):
        rec = np.searchsorted(starts, p, side="right") - 1          # the last record that starts at or before p
        for a in range(0, len(p), 512):
            pa, ra = p[a:a + 512, None], rec[a:a + 512]
            length = q[None, :] + k - pa
            ok = (q[None, :] >= pa) & (length >= min_len) & (length <= max_len)
            ok &= (ra >= 0)[:, None] & (q[None, :] + k <= ends[np.maximum(ra, 0)][:, None])
            i, j = np.nonzero(ok)
            part = np.zeros(len(i), dtype=AMPLICON_DTYPE)
            part["fwd"], part["rev"] = plus["primer"][a + i], minus["primer"][j]
            part["pos"], part["len"] = p[a + i], length[i, j]
            out.append(part)
    amps = np.concatenate(out) if out else np.zeros(0, dtype=AMPLICON_DTYPE)
    amps = amps[np.lexsort((amps["rev"], amps["fwd"], amps["len"], amps["pos"]))]
    counts = np.zeros((n, 2), dtype=np.uint64)
    np.add.at(counts[:, 0], amps["fwd"].astype(np.int64), 1)
    np.add.at(counts[:, 1], amps["rev"].astype(np.int64), 1)
    return counts, len(amps), amps


def amplicons_of(n: int, k: int, scored, records, min_len: int, max_len: int):
    """The same from the scored-site model's records (SCORED_SITE_DTYPE): the stable ones are paired."""
    return pair_sites(n, k, scored[scored["stable"] != 0], records, min_len, max_len)


def amplicons(tables, records, primers, M: int, E: int, mode, tm_threshold: float, min_len: int, max_len: int,
              args=None, scored=None):
    """(site counts, stable counts, amplicon counts (n, 2), total, sorted list).  scored: the result of
    background_thal_model.scored_sites for the same arguments, when the caller has it already."""
    primers = list(primers)
    k = len(primers[0]) if primers else 0
    counts, stable, recs = scored if scored is not None else btm.scored_sites(tables, records, primers, M, E, mode,
                                                                              tm_threshold, args)
    amp_counts, total, amps = amplicons_of(len(primers), k, recs, records, min_len, max_len)
    return counts, stable, amp_counts, total, amps


def render(names, record_names, records, amp_counts, amps, min_len: int, max_len: int) -> str:
    """The block od-msspe-hip --background ... --background-tm ... --background-amplicon-max prints after the scored
    block."""
    starts, _total = bm.record_starts(records)
    c = np.asarray(amp_counts, dtype=np.uint64).reshape(-1, 2)
    out = f"\nBackground amplicons (stable sites facing each other, {min_len} to {max_len} bases):\n"
    for nm, (f, r) in zip(names, c.tolist()):
        out += f"  {nm}: as forward {f}, as reverse {r}\n"
    out += f"  Total: {len(c)} primers, {int(c[:, 0].sum())} amplicons\n"
    shown = amps[:20]
    out += f"  First {len(shown)} (record:offset, length, forward, reverse):\n"
    for a in shown:
        r = int(np.searchsorted(starts, int(a["pos"]), side="right")) - 1
        out += (f"    {record_names[r]}:{int(a['pos']) - int(starts[r])}, {int(a['len'])}, {names[int(a['fwd'])]}, "
                f"{names[int(a['rev'])]}\n")
    return out
