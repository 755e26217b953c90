"""Restatement of msspe_segment_coverage_thal* (include/msspe_hip.h), written from its semantics on top of the numpy
model of coverage within N mismatches (tests/coverage_mm_model.py: window_kmers, _match), the CPU oracle's thal
(oracle/pyoracle.py) and the background screen's stable rule (tests/background_thal_model.py is_stable).

A MATCH is (segment s = r * P + j, primer q, window position p) that the mm rule accepts; q runs over the forward
primers, then the reverse primers.  A forward primer is compared in the head window, a reverse primer against the
reverse complement of the tail window's k columns.  The TEMPLATE OLIGO o2 is the strand the primer anneals to, 5'->3':
revcomp(head columns at p) for a forward primer, the tail columns at p as written for a reverse primer.  The score is
thal(u, o2), mode 1 ANY or 2 END1; raw dG is +inf and raw t is 0 without a structure.  t_match = max(0, t); the match is
STABLE iff not (round_fixed_f32(t_match, 2) < float32(tm_threshold)).  held: 0 no match, 1 matches but none stable, 2 a
stable match; t_best: the greatest t_match of the segment, 0.0 without a match.  Also renders the block od-msspe-hip
--coverage-tm prints."""
from __future__ import annotations

import numpy as np

import coverage_mm_model as cm
import pyoracle
from background_thal_model import MODES, is_stable

SCORED_MATCH_DTYPE = np.dtype([("primer", np.uint32), ("segment", np.uint32), ("offset", np.uint32),
                               ("mismatches", np.uint16), ("stable", np.uint16), ("dg", np.float64),
                               ("t", np.float64)])
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def _prim(words, k):
    return cm.codes(list(words)).reshape(len(words), k) if len(words) else np.zeros((0, k), dtype=np.int8)


def matches(seqs, seg: int, stride: int, W: int, k: int, fwd, rev, M: int, E: int, chunk: int = 64):
    """(records without scores, template oligos): every match, sorted by (primer, segment, offset), and the strand
    each primer anneals to there, cut from the alignment's own columns."""
    a = np.ascontiguousarray(seqs, dtype=np.uint8)
    n, L = a.shape
    P = cm.n_partitions(L, seg, stride)
    segments = [(r, j) for r in range(n) for j in range(P)]
    F, R = _prim(fwd, k), _prim(rev, k)
    rows = []
    for at in range(0, len(segments), chunk):
        head, tail = cm.window_kmers(a, seg, stride, W, k, segments[at:at + chunk])
        for cand, prim, first, is_rev in ((head, F, 0, False), (tail, R, len(F), True)):
            mm, hit = cm._match(cand, prim, M, E)
            for sl, p, q in np.argwhere(hit):
                r, j = segments[at + sl]
                col = j * stride + (seg - W if is_rev else 0) + int(p)
                cols = bytes(a[r, col:col + k]).decode()
                rows.append((first + int(q), r * P + j, int(p), int(mm[sl, p, q]), cols if is_rev else revcomp(cols)))
    rows.sort(key=lambda x: x[:3])
    recs = np.zeros(len(rows), dtype=SCORED_MATCH_DTYPE)
    for f, col in (("primer", 0), ("segment", 1), ("offset", 2), ("mismatches", 3)):
        recs[f] = [x[col] for x in rows]
    return recs, [x[4] for x in rows]


def score(tables, primers, recs, o2, mode, args=None, cache=None):
    """The oracle's raw doubles of every match; thal is a pure function of (primer, template), so a cache is exact."""
    mode = MODES[mode] if isinstance(mode, str) else mode
    cache = {} if cache is None else cache
    dg, t = np.empty(len(recs)), np.empty(len(recs))
    for i, (r, b) in enumerate(zip(recs, o2)):
        key = (primers[int(r["primer"])], b, mode)
        if key not in cache:
            res = pyoracle.thal(tables, key[0], key[1], mode, args)
            cache[key] = (np.inf, 0.0) if res.no_structure else (res.dG, res.t)
        dg[i], t[i] = cache[key]
    return dg, t


def fold(recs, n_seg: int, n_primers: int):
    """held uint8, t_best float64 (n_seg each), primer_segments and primer_held uint32 from scored records."""
    held = np.zeros(n_seg, dtype=np.uint8)
    t_best = np.zeros(n_seg, dtype=np.float64)
    seen, seen_held = set(), set()
    for r in recs:
        s, q, t = int(r["segment"]), int(r["primer"]), float(r["t"])
        held[s] = max(held[s], 2 if r["stable"] else 1)
        t_best[s] = max(t_best[s], t if t > 0.0 else 0.0)
        seen.add((q, s))
        if r["stable"]:
            seen_held.add((q, s))
    primer_segments = np.zeros(n_primers, dtype=np.uint32)
    primer_held = np.zeros(n_primers, dtype=np.uint32)
    for q, _ in seen:
        primer_segments[q] += 1
    for q, _ in seen_held:
        primer_held[q] += 1
    return held, t_best, primer_segments, primer_held


def coverage_thal(tables, seqs, seg: int, stride: int, W: int, k: int, fwd, rev, M: int, E: int, mode,
                  tm_threshold: float, args=None, chunk: int = 64, cache=None) -> dict:
    """What Engine.segment_coverage_thal(..., matches=True) returns, from the model."""
    a = np.ascontiguousarray(seqs, dtype=np.uint8)
    n, L = a.shape
    P = cm.n_partitions(L, seg, stride)
    primers = list(fwd) + list(rev)
    recs, o2 = matches(a, seg, stride, W, k, fwd, rev, M, E, chunk)
    recs["dg"], recs["t"] = score(tables, primers, recs, o2, mode, args, cache)
    recs["stable"] = [is_stable(float(t), tm_threshold) for t in recs["t"]]
    held, t_best, ps, ph = fold(recs, n * P, len(primers))
    return {"held": held.reshape(n, P), "t_best": t_best.reshape(n, P), "primer_segments": ps, "primer_held": ph,
            "matches": recs, "count": len(recs), "templates": o2}


def rethreshold(result: dict, tm_threshold: float) -> dict:
    """The same matches and scores judged at another threshold."""
    recs = result["matches"].copy()
    recs["stable"] = [is_stable(float(t), tm_threshold) for t in recs["t"]]
    shape = result["held"].shape
    held, t_best, ps, ph = fold(recs, shape[0] * shape[1], len(result["primer_held"]))
    return {**result, "held": held.reshape(shape), "t_best": t_best.reshape(shape), "primer_segments": ps,
            "primer_held": ph, "matches": recs}


def render(names, lengths, held: np.ndarray, primer_held, seg: int, stride: int, M: int, E: int, mode,
           tm_threshold: float) -> str:
    """The block od-msspe-hip --coverage-tm prints, from held (n_seq, P) and the per-primer held counts: f32
    arithmetic and %.1f as the other coverage blocks.  lengths: each record's own length."""
    total = n_held = matched = 0
    seq_stats = {}
    for r, (name, ln) in enumerate(zip(names, lengths)):
        se = seq_stats.setdefault(name, [0, 0])
        for j in range(cm.n_partitions(ln, seg, stride)):
            h = int(held[r, j])
            se[1] += 1
            total += 1
            matched += h != 0
            if h == 2:
                se[0] += 1
                n_held += 1
    covs = [np.float32(c) / np.float32(t) * np.float32(100.0) for c, t in seq_stats.values()]
    name = {1: "ANY", 2: "END1", "any": "ANY", "end1": "END1"}[mode]
    out = "\nCoverage report (thal %s, t >= %.2f C; matches within %d mismatches, last %d bases exact):\n" % (
        name, float(np.float32(tm_threshold)), M, E)
    out += "  Segments:  %d/%d held (%.1f%%), %d/%d matched\n" % (
        n_held, total, float(np.float32(100.0) * np.float32(n_held) / np.float32(total)), matched, total)
    out += "  Sequences: %d/%d at ≥80%% held (min %.1f%%, max %.1f%%)\n" % (
        sum(1 for c in covs if c >= 80.0), len(seq_stats), float(min(covs)), float(max(covs)))
    ph = np.asarray(primer_held)
    out += "  Primers:   %d of %d hold no segment\n" % (int((ph == 0).sum()), len(ph))
    return out
