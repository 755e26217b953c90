"""numpy restatement of the background screen (msspe_background_sites*, include/msspe_hip.h), written from its
semantics: sites of every primer on both strands of a stream of unaligned records, within M mismatches with the primer's
last E bases exact.  Also renders the block od-msspe-hip --background prints.

The stream is the records back to back with one invalid column between two; only upper-case A C G T are bases.  For
every stream position p and primer u (primer orientation): a PLUS site when the k columns at p are all bases and differ
from u at <= M positions, none of them among u's last E; a MINUS site when the reverse complement of those k columns
does.  Cost: a few passes over the stream per primer (bit planes of every window, XOR / OR / popcount per primer)."""
from __future__ import annotations

import numpy as np

SITE_DTYPE = np.dtype([("primer", np.uint32), ("pos", np.uint32), ("mismatches", np.uint16), ("strand", np.uint16)])
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def record_starts(records) -> tuple[np.ndarray, int]:
    """(first stream column of each record, total stream length)."""
    starts, at = [], 0
    for i, r in enumerate(records):
        if i:
            at += 1
        starts.append(at)
        at += len(r)
    return np.array(starts, dtype=np.uint64), at


def stream_codes(records) -> np.ndarray:
    """The stream as codes: A 0, C 1, G 2, T 3, anything else (and the separators) 4."""
    _starts, total = record_starts(records)
    out = np.full(total, 4, dtype=np.uint8)
    at = 0
    for i, r in enumerate(records):
        if i:
            at += 1
        b = r.encode() if isinstance(r, str) else bytes(r)
        out[at:at + len(b)] = _CODE[np.frombuffer(b, dtype=np.uint8)]
        at += len(b)
    return out


def _planes(codes: np.ndarray, k: int):
    """Per window position: (low plane, high plane, all-bases flag); bit q of a plane belongs to the window's base q."""
    n = len(codes) - k + 1
    lo = np.zeros(n, dtype=np.uint32)
    hi = np.zeros(n, dtype=np.uint32)
    ok = np.ones(n, dtype=bool)
    for q in range(k):
        c = codes[q:q + n]
        lo |= (c & 1).astype(np.uint32) << np.uint32(q)
        hi |= ((c >> 1) & 1).astype(np.uint32) << np.uint32(q)
        ok &= c < 4
    return lo, hi, ok


def _primer_planes(p: str):
    lo = hi = 0
    for q, ch in enumerate(p):
        c = "ACGT".index(ch)
        lo |= (c & 1) << q
        hi |= (c >> 1) << q
    return np.uint32(lo), np.uint32(hi)


def candidates(records, primers, max_m: int) -> np.ndarray:
    """Every (primer, strand, pos) whose window holds k bases and differs from the primer (plus) / whose reverse
    complement differs from it (minus) at <= max_m positions, whatever their place: a structured array with the
    fields of SITE_DTYPE and "mask" (bit q: the primer's base q differs).  sites() filters it by (M, E), so one pass
    serves a grid of them."""
    primers = list(primers)
    dt = np.dtype(SITE_DTYPE.descr + [("mask", np.uint32)])
    if not primers:
        return np.zeros(0, dtype=dt)
    k = len(primers[0])
    codes = stream_codes(records)
    if len(codes) < k:
        return np.zeros(0, dtype=dt)
    full = np.uint32((1 << k) - 1)
    lo, hi, ok = _planes(codes, k)
    # the reverse complement of each window: base q = complement of the window's base k - 1 - q
    n = len(lo)
    rlo = np.zeros(n, dtype=np.uint32)
    rhi = np.zeros(n, dtype=np.uint32)
    for q in range(k):
        rlo |= ((lo >> np.uint32(k - 1 - q)) & np.uint32(1)) << np.uint32(q)
        rhi |= ((hi >> np.uint32(k - 1 - q)) & np.uint32(1)) << np.uint32(q)
    rlo, rhi = ~rlo & full, ~rhi & full
    out = []
    for i, p in enumerate(primers):
        assert len(p) == k
        ulo, uhi = _primer_planes(p)
        for strand, (a, b) in enumerate(((lo, hi), (rlo, rhi))):
            d = (a ^ ulo) | (b ^ uhi)
            pc = np.bitwise_count(d)
            at = np.flatnonzero(ok & (pc <= max_m))
            rec = np.zeros(len(at), dtype=dt)
            rec["primer"], rec["pos"], rec["mismatches"], rec["strand"], rec["mask"] = i, at, pc[at], strand, d[at]
            out.append(rec)
    return np.concatenate(out)


def sites(records, primers, M: int, E: int, cand: np.ndarray | None = None):
    """(counts uint64 (n, 2): plus / minus sites per primer, sites: SITE_DTYPE array sorted by (primer, strand, pos)).
    cand: candidates(records, primers, max_m) with max_m >= M, when a grid of (M, E) shares it."""
    primers = list(primers)
    k = len(primers[0]) if primers else 0
    if cand is None:
        cand = candidates(records, primers, M)
    keep = cand["mismatches"] <= M
    if E:
        keep &= (cand["mask"] >> np.uint32(k - E)) == 0   # no differing base among the primer's last E
    c = cand[keep]
    out = np.zeros(len(c), dtype=SITE_DTYPE)
    for f in SITE_DTYPE.names:
        out[f] = c[f]
    out = out[np.lexsort((out["pos"], out["strand"], out["primer"]))]
    counts = np.zeros((len(primers), 2), dtype=np.uint64)
    np.add.at(counts, (out["primer"].astype(np.int64), out["strand"].astype(np.int64)), 1)
    return counts, out


def naive_sites(records, primers, M: int, E: int):
    """The semantics as a string-compare triple loop (tiny inputs only): the same two outputs as sites()."""
    primers = list(primers)
    k = len(primers[0]) if primers else 0
    stream = "-".join(r if isinstance(r, str) else bytes(r).decode("latin-1") for r in records)
    out = []
    for i, u in enumerate(primers):
        for strand in (0, 1):
            for p in range(len(stream) - k + 1):
                w = stream[p:p + k]
                if any(ch not in "ACGT" for ch in w):
                    continue
                if strand:
                    w = revcomp(w)
                diff = [q for q in range(k) if w[q] != u[q]]
                if len(diff) <= M and all(q < k - E for q in diff):
                    out.append((i, p, len(diff), strand))
    arr = np.array(out, dtype=SITE_DTYPE) if out else np.zeros(0, dtype=SITE_DTYPE)
    counts = np.zeros((len(primers), 2), dtype=np.uint64)
    for i, _p, _m, s in out:
        counts[i, s] += 1
    return counts, arr


def render(names, counts, M: int, E: int) -> str:
    """The block od-msspe-hip --background prints after the coverage report."""
    out = f"\nBackground sites (up to {M} mismatches, last {E} bases exact):\n"
    for name, (plus, minus) in zip(names, np.asarray(counts).tolist()):
        out += f"  {name}: plus {plus}, minus {minus}\n"
    c = np.asarray(counts, dtype=np.uint64).reshape(-1, 2)
    out += f"  Total: {len(c)} primers, plus {int(c[:, 0].sum())}, minus {int(c[:, 1].sum())}\n"
    return out
