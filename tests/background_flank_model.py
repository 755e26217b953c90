"""Restatement of msspe_background_thal_flank* / msspe_background_amplicons_flank* (include/msspe_hip.h), written from
their semantics on top of the site model (tests/background_model.py), the scored-site model
(tests/background_thal_model.py) and the CPU oracle's thal (oracle/pyoracle.py).

A site {primer u, pos p, strand s} of the string rule and a flank f (0 <= f <= 4, k + 2 f <= 32): fl is the number of
consecutive base columns (upper-case A C G T) that end at column p - 1, capped at f, and fr the number that start at
column p + k, capped at f; anything else -- N, IUPAC codes, lower case, '-', the separator between two records, the
ends of the stream -- stops the count.  The EXTENDED WINDOW is W = stream[p - fl, p + k + fr) and the TEMPLATE OLIGO is
revcomp(W) on the plus strand (0) and W on the minus strand (1), k + fl + fr bases.  The site score is thal(u, o2);
sites, mismatch counts, t_site and the stable rule are those of flank 0, which is the scored-site model itself."""
from __future__ import annotations

import numpy as np

import background_model as bm
import background_thal_model as btm

MAX_FLANK = 4


def flanks(stream: str, k: int, pos: int, f: int) -> tuple[int, int]:
    """(fl, fr) of the window of k columns at pos."""
    assert 0 <= f <= MAX_FLANK and k + 2 * f <= 32
    fl = 0
    while fl < f and pos - 1 - fl >= 0 and stream[pos - 1 - fl] in "ACGT":
        fl += 1
    fr = 0
    while fr < f and pos + k + fr < len(stream) and stream[pos + k + fr] in "ACGT":
        fr += 1
    return fl, fr


def template_oligo(stream: str, k: int, pos: int, strand: int, f: int) -> str:
    fl, fr = flanks(stream, k, pos, f)
    w = stream[pos - fl:pos + k + fr]
    return w if strand else bm.revcomp(w)


def template_oligos(records, primers, sites, f: int) -> list[str]:
    k = len(primers[0]) if len(primers) else 0
    s = btm.stream_text(records)
    return [template_oligo(s, k, int(r["pos"]), int(r["strand"]), f) for r in sites]


def site_classes(records, primers, sites, f: int) -> np.ndarray:
    """(len(sites), 2) int array of (fl, fr)."""
    k = len(primers[0]) if len(primers) else 0
    s = btm.stream_text(records)
    return np.array([flanks(s, k, int(r["pos"]), f) for r in sites], dtype=np.int64).reshape(-1, 2)


def class_stats(records, primers, sites, f: int) -> tuple[int, int]:
    """(distinct (fl, fr) classes among the sites, sites with fl < f or fr < f): what msspe_get_info reports as
    "background_thal_flank_classes" and "background_thal_truncated"."""
    c = site_classes(records, primers, sites, f)
    return len({tuple(x) for x in c.tolist()}), int(((c[:, 0] < f) | (c[:, 1] < f)).sum())


def scored_sites(tables, records, primers, M: int, E: int, mode, tm_threshold: float, args=None, flank: int = 0):
    """(counts (n, 2), stable (n, 2), records sorted by (primer, strand, pos)) at the given flank."""
    primers = list(primers)
    counts, sites = bm.sites(records, primers, M, E)
    o2 = template_oligos(records, primers, sites, flank)
    dg, t = btm.score(tables, primers, sites, o2, mode, args)
    recs = btm.records_of(sites, dg, t, tm_threshold)
    return counts, btm.stable_counts(len(primers), recs), recs


def render(names, counts, stable, M: int, E: int, mode, tm_threshold: float, flank: int = 0) -> str:
    """The block od-msspe-hip --background ... --background-tm ... --background-flank prints: the scored block, its
    header line extended by ", template flank <f>" behind the threshold when f > 0."""
    text = btm.render(names, counts, stable, M, E, mode, tm_threshold)
    if flank > 0:
        head, rest = text[1:].split("\n", 1)
        assert head.endswith(" C):")
        text = "\n" + head[:-2] + f", template flank {flank}):\n" + rest
    return text
