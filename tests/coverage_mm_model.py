"""numpy restatement of segment coverage within N mismatches, the primer's 3' end exact (msspe_segment_coverage_mm,
include/msspe_hip.h), for small inputs: sliding windows and broadcast comparisons.  Also renders the block
od-msspe-hip --coverage-mismatches prints.

Segments are those of the exact report (od-msspe/src/main.rs:518-594): segment (r, j) starts at column j * stride,
its head window is its first W columns, its tail window its last W.  For each position p in [0, W - k] the forward
candidate is the head window's k bases at p, the reverse candidate the reverse complement of the tail window's k bases
at p.  A candidate holding anything but A / C / G / T never matches.  It matches a primer of its direction when they
differ at <= M base positions and agree on the primer's last E bases."""
from __future__ import annotations

import numpy as np

_CODE = np.full(256, -1, dtype=np.int8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def codes(x) -> np.ndarray:
    """Strings, a uint8 matrix or a list of equal-length strings -> int8 codes (A 0, C 1, G 2, T 3, other -1)."""
    if isinstance(x, np.ndarray):
        return _CODE[x]
    if isinstance(x, str):
        return _CODE[np.frombuffer(x.encode(), dtype=np.uint8)]
    if len(x) == 0:
        return np.zeros((0, 0), dtype=np.int8)
    return _CODE[np.frombuffer("".join(x).encode(), dtype=np.uint8).reshape(len(x), -1)]


def n_partitions(L: int, seg: int, stride: int) -> int:
    return 0 if L < seg else (L - seg) // stride + 1


def window_kmers(seqs: np.ndarray, seg: int, stride: int, W: int, k: int, segments=None):
    """(head, tail) int8 arrays (n_segments, W - k + 1, k): the forward candidates and the reverse candidates (tail
    k-mers reverse-complemented; -1 stays -1) of the given segments (r, j) -- all of them, r-major, by default."""
    c = codes(np.ascontiguousarray(seqs, dtype=np.uint8))
    n, L = c.shape
    P = n_partitions(L, seg, stride)
    if segments is None:
        segments = [(r, j) for r in range(n) for j in range(P)]
    seg_arr = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    per = W - k + 1
    offs = np.arange(per)[:, None] + np.arange(k)[None, :]            # (per, k)
    col0 = seg_arr[:, 1] * stride
    rows = seg_arr[:, 0][:, None, None]
    head = c[rows, col0[:, None, None] + offs[None]]
    tail = c[rows, (col0 + seg - W)[:, None, None] + offs[None]][:, :, ::-1]
    tail = np.where(tail >= 0, 3 - tail, -1).astype(np.int8)
    return head, tail


def _match(cand: np.ndarray, prim: np.ndarray, M: int, E: int):
    """cand (S, per, k), prim (n, k) -> (mismatch counts (S, per, n), match bits (S, per, n))."""
    k = cand.shape[-1]
    if prim.shape[0] == 0:
        z = np.zeros(cand.shape[:2] + (0,), dtype=np.int64)
        return z, z.astype(bool)
    diff = cand[:, :, None, :] != prim[None, None, :, :]
    mm = diff.sum(-1)
    ok3 = ~diff[..., k - E:].any(-1) if E else np.ones(mm.shape, dtype=bool)
    valid = (cand >= 0).all(-1)[:, :, None]
    return mm, valid & ok3 & (mm <= M)


def best_and_counts(seqs: np.ndarray, seg: int, stride: int, W: int, k: int, fwd, rev, M: int, E: int,
                    segments=None, chunk: int = 64):
    """best uint8 (n_segments,) -- the smallest mismatch count of a match, 255 when none -- and counts uint32
    (len(fwd) + len(rev),): segments each primer matches in (restricted to `segments` when given)."""
    F = codes(list(fwd)).reshape(len(fwd), k) if len(fwd) else np.zeros((0, k), dtype=np.int8)
    R = codes(list(rev)).reshape(len(rev), k) if len(rev) else np.zeros((0, k), dtype=np.int8)
    c = np.ascontiguousarray(seqs, dtype=np.uint8)
    n, L = c.shape
    P = n_partitions(L, seg, stride)
    if segments is None:
        segments = [(r, j) for r in range(n) for j in range(P)]
    best = np.full(len(segments), 255, dtype=np.uint8)
    counts = np.zeros(len(F) + len(R), dtype=np.uint32)
    for a in range(0, len(segments), chunk):
        head, tail = window_kmers(c, seg, stride, W, k, segments[a:a + chunk])
        b = np.full(head.shape[0], 255, dtype=np.int64)
        for cand, prim, off in ((head, F, 0), (tail, R, len(F))):
            mm, hit = _match(cand, prim, M, E)
            if prim.shape[0]:
                b = np.minimum(b, np.where(hit, mm, 255).min(axis=(1, 2)))
                counts[off:off + len(prim)] += hit.any(axis=1).sum(axis=0).astype(np.uint32)
        best[a:a + chunk] = b
    return best, counts


def best_matrix(seqs: np.ndarray, seg: int, stride: int, W: int, k: int, fwd, rev, M: int, E: int, chunk: int = 64):
    """best as the C call returns it: uint8 (n_seq, P), and the counts."""
    n, L = np.asarray(seqs).shape
    P = n_partitions(L, seg, stride)
    best, counts = best_and_counts(seqs, seg, stride, W, k, fwd, rev, M, E, chunk=chunk)
    return best.reshape(n, P), counts


def render_block(names, lengths, best: np.ndarray, seg: int, stride: int, M: int, E: int) -> str:
    """The text od-msspe-hip --coverage-mismatches M --coverage-3p-exact E appends to the exact report, from
    best (n_seq, P): the exact report's three lines (main.rs:574-593, f32 arithmetic) with hit = best <= M, then the
    segments by best mismatch count.  lengths: each record's own length (segments past it are not counted)."""
    total = covered = 0
    seq_stats, part_stats = {}, {}
    by = [0] * (M + 2)
    for r, (name, ln) in enumerate(zip(names, lengths)):
        se = seq_stats.setdefault(name, [0, 0])
        for j in range(n_partitions(ln, seg, stride)):
            b = int(best[r, j])
            hit = b <= M
            pe = part_stats.setdefault(j & 0xFFFF, [0, 0])
            se[1] += 1
            pe[1] += 1
            total += 1
            by[min(b, M + 1)] += 1
            if hit:
                se[0] += 1
                pe[0] += 1
                covered += 1
    covs = [np.float32(c) / np.float32(t) * np.float32(100.0) for c, t in seq_stats.values()]
    out = "\nCoverage report (up to %d mismatches, last %d bases exact):\n" % (M, E)
    out += "  Segments:  %d/%d covered (%.1f%%)\n" % (
        covered, total, float(np.float32(100.0) * np.float32(covered) / np.float32(total)))
    out += "  Sequences: %d/%d at ≥80%% coverage (min %.1f%%, max %.1f%%)\n" % (
        sum(1 for c in covs if c >= 80.0), len(seq_stats), float(min(covs)), float(max(covs)))
    unc = sorted(p for p, (c, _) in part_stats.items() if c == 0)
    out += "  All partitions have primer coverage\n" if not unc else \
        "  Uncovered partitions: [%s]\n" % ", ".join(str(p) for p in unc)
    out += "  Segments by best match:" + "".join(" %d mm %d," % (m, by[m]) for m in range(M + 1)) + \
        " none %d\n" % by[M + 1]
    return out
