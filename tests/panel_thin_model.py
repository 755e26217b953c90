"""numpy restatement of the panel thinning (msspe_panel_thin, include/msspe_hip.h) for small inputs.

Incidence: I[p][s] is True when primer p (forward primers first, then reverse, in the caller's order) has at least one
match in segment s = r * P + j under the rule of coverage_mm_model: a forward primer in the head window, a reverse
primer in the tail window against the reverse-complemented candidate, at most M differing positions, the primer's last
E bases exact, a candidate holding anything but A / C / G / T never a match.

Greedy: forced primers cover first and are never picked.  Every round takes the unforced, unpicked primer with the
most uncovered segments, ties to the lowest index; below min_gain the loop ends and nothing is picked in that round."""
from __future__ import annotations

import numpy as np

from coverage_mm_model import _match, codes, n_partitions, window_kmers


def incidence(seqs: np.ndarray, seg: int, stride: int, W: int, k: int, fwd, rev, M: int, E: int,
              chunk: int = 64) -> np.ndarray:
    """bool (len(fwd) + len(rev), n_seq * P)."""
    F = codes(list(fwd)).reshape(len(fwd), k) if len(fwd) else np.zeros((0, k), dtype=np.int8)
    R = codes(list(rev)).reshape(len(rev), k) if len(rev) else np.zeros((0, k), dtype=np.int8)
    c = np.ascontiguousarray(seqs, dtype=np.uint8)
    n, L = c.shape
    P = n_partitions(L, seg, stride)
    segments = [(r, j) for r in range(n) for j in range(P)]
    I = np.zeros((len(F) + len(R), len(segments)), dtype=bool)
    for a in range(0, len(segments), chunk):
        head, tail = window_kmers(c, seg, stride, W, k, segments[a:a + chunk])
        for cand, prim, off in ((head, F, 0), (tail, R, len(F))):
            if prim.shape[0]:
                _, hit = _match(cand, prim, M, E)
                I[off:off + len(prim), a:a + head.shape[0]] = hit.any(axis=1).T
    return I


def greedy(I: np.ndarray, min_gain: int = 1, forced=None):
    """(keep uint8[n], order, gains, covered bool[N_s], covered_all, covered_kept, rounds): rounds counts the picks and
    the round that stopped."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    covered = I[forced].any(axis=0) if forced.any() else np.zeros(n_seg, dtype=bool)
    live = ~forced
    order, gains = [], []
    rounds = 0
    while True:
        rounds += 1
        g = np.where(live, (I & ~covered).sum(axis=1), -1) if n else np.zeros(0, dtype=np.int64)
        if n == 0 or g.max() < min_gain:   # nobody live: max is -1
            break
        p = int(np.argmax(g))              # the first maximum: the lowest index
        order.append(p)
        gains.append(int(g[p]))
        live[p] = False
        covered = covered | I[p]
    keep = forced.copy()
    keep[np.array(order, dtype=np.int64)] = True
    return (keep.astype(np.uint8), np.array(order, dtype=np.uint32), np.array(gains, dtype=np.uint32), covered,
            int(I.any(axis=0).sum()) if n else 0, int(covered.sum()), rounds)


def pack_rows(I: np.ndarray) -> np.ndarray:
    """bool (n, N_s) -> uint64 (n, ceil(N_s / 64)), bit s & 63 of word s >> 6: what odm_thin_panel reads."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    words = max(1, (n_seg + 63) // 64)
    padded = np.zeros((n, words * 64), dtype=np.uint8)
    padded[:, :n_seg] = I
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n, words))


def render_block(M: int, E: int, G: int, kept_f: int, n_f: int, kept_r: int, n_r: int, forced: int,
                 covered_all: int, covered_kept: int, segments: int) -> str:
    """The text od-msspe-hip --thin-panel true prints after the coverage report(s).  The primer figures leave the
    forced primers (the panel of --existing-primers) out; the segment figures include what they cover; segments is
    rows * P of the alignment as uploaded."""
    x, y = kept_f + kept_r, n_f + n_r
    return ("\nPanel thinning (up to %d mismatches, last %d bases exact, gain >= %d):\n" % (M, E, G) +
            "  Primers:  kept %d of %d (forward %d of %d, reverse %d of %d), %d forced\n" % (
                x, y, kept_f, n_f, kept_r, n_r, forced) +
            "  Segments: covered %d/%d by all %d, %d/%d by the kept %d\n" % (
                covered_all, segments, y, covered_kept, segments, x))
