"""The model of the conflict graph under a pair of rules (msspe_conflict_graph*), on the CPU oracle.

ANY: Primer3 2.6.1 thal ANY per ordered pair, decided by the reference's two filters on dG (pyoracle.edge_decision).
END: thal END1 per ordered pair (the row is oligo 1, the anchored 3' end), decided by od-msspe's SELF_END rule applied
to the pair: conflict iff !(round_fixed_f32(max(0, t), 2) < threshold).
The graph: a pair conflicts under at least one enabled rule.  Row counts count a pair under both rules once; the kind
counts are the pairs that are ANY only, END only and both; the edge list is every conflicting pair as (a, b, kinds) in
ascending (a, b) order.  Nothing here runs on the GPU, and the planes of a pool are computed once per process."""
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np

KIND_ANY, KIND_END = 1, 2
KIND_EDGE = np.dtype([("a", np.uint32), ("b", np.uint32), ("kinds", np.uint32), ("reserved", np.uint32)])

# (k, n, dG threshold, END Tm threshold) of the pools the tests share, with the kinds each holds at ntthal's
# defaults: ANY only, END only, both
POOL_RULES = [
    ((13, 160, -12000.0, 25.0), (11, 35, 11)),
    ((13, 160, -9000.0, 10.0), (189, 171, 114)),
    ((13, 65, -12000.0, 25.0), (8, 10, 10)),
    ((20, 96, -12000.0, 25.0), (40, 24, 58)),
]


def rand_oligos(rng, n, k, alphabet="ACGT"):
    return ["".join(alphabet[x] for x in rng.integers(0, len(alphabet), k)) for _ in range(n)]


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def end_pool(k, n, seed):
    """Random oligos of length k with the shapes END1 cares about: self-complementary oligos (even k), partners that
    pair with another oligo's 3' end, and pairs whose last DP row is empty (oligo 1 ends in A, the partner holds no
    T) with and without a base pair at cell (1, 1)."""
    rng = np.random.default_rng(seed * 100 + k)
    P = rand_oligos(rng, n, k)
    for j in range(0, min(16, n // 4)):          # 3'-complementary partners
        a = P[j]
        tail = a[-min(k, max(2, (3 * k) // 4)):]
        P[n // 2 + j] = (rc(tail) + P[n // 2 + j])[:k]
    if k % 2 == 0:                               # self-complementary oligos
        for j in range(6):
            h = rand_oligos(rng, 1, k // 2)[0]
            P[n // 4 + j] = h + rc(h)
    for j in range(4):                           # empty last row: oligo 1 = ...A, partners without T
        a = "C" + rand_oligos(rng, 1, k - 2, "ACG")[0] + "A" if k > 2 else "CA"
        with_bp = rand_oligos(rng, 1, k - 1, "ACG")[0] + "G"
        without = rand_oligos(rng, 1, k - 1, "ACG")[0] + "A"
        P[n - 1 - 3 * j], P[n - 2 - 3 * j], P[n - 3 - 3 * j] = a, with_bp[-k:], without[-k:]
    return P


def distinct(pool):
    """The pool with every repeated oligo replaced: its first base is rotated (A -> C -> G -> T -> A) until the oligo
    is new.  The graph consumers refuse duplicates."""
    seen, out = set(), []
    for s in pool:
        while s in seen:
            s = "ACGT"[("ACGT".index(s[0]) + 1) % 4] + s[1:]
        seen.add(s)
        out.append(s)
    return out


def shared_pool(k, n):
    return distinct(end_pool(k, n, 7))


def chem_args(oracle, chem_name):
    return oracle.ntthal_args() if chem_name == "ntthal" else oracle.p3_args()


def any_rule(oracle, dg, thr):
    """The reference's decision on a thal ANY dG (+inf: no structure, no edge)."""
    out = np.zeros(dg.shape, dtype=np.uint8)
    for idx, v in np.ndenumerate(dg):
        out[idx] = np.isfinite(v) and oracle.edge_decision(float(v), thr)
    return out


def end_rule(oracle, t, thr):
    """od-msspe's SELF_END rule on a pair: conflict iff !(round_fixed_f32(t_end, 2) < thr), t_end = max(0, t)."""
    thr32 = float(np.float32(thr))
    te = np.maximum(t, 0.0)
    out = np.zeros(te.shape, dtype=np.uint8)
    for idx, v in np.ndenumerate(te):
        out[idx] = not oracle.round_fixed_f32(float(v), 2) < thr32
    return out


@lru_cache(maxsize=None)
def _raw_square(k, n, chem_name):
    import pyoracle as oracle
    tables = oracle.Tables()
    pool = shared_pool(k, n)
    args = chem_args(oracle, chem_name)
    _, dg, _, _ = oracle.pool_pairs(tables, pool, args, 0.0, mode=oracle.ANY, want_conflict=False)
    _, _, _, tt = oracle.pool_pairs(tables, pool, args, 0.0, mode=oracle.END1, want_dg=False, want_conflict=False,
                                    want_t=True)
    return pool, dg, tt


@lru_cache(maxsize=None)
def square_planes(k, n, dg_thr, tm_thr, chem_name="ntthal"):
    """(pool, ANY decisions, END decisions) of shared_pool(k, n): uint8 (n, n) each, read-only."""
    import pyoracle as oracle
    pool, dg, tt = _raw_square(k, n, chem_name)
    a, e = any_rule(oracle, dg, dg_thr), end_rule(oracle, tt, tm_thr)
    a.setflags(write=False)
    e.setflags(write=False)
    return pool, a, e


def random_planes(oracle, tables, pool, dg_thr, tm_thr):
    """(ANY decisions, END decisions) of any pool of one length at ntthal's defaults."""
    args = oracle.ntthal_args()
    _, dg, _, _ = oracle.pool_pairs(tables, pool, args, 0.0, mode=oracle.ANY, want_conflict=False)
    _, _, _, tt = oracle.pool_pairs(tables, pool, args, 0.0, mode=oracle.END1, want_dg=False, want_conflict=False,
                                    want_t=True)
    return any_rule(oracle, dg, dg_thr), end_rule(oracle, tt, tm_thr)


def ab_planes(oracle, tables, A, B, dg_thr, tm_thr, args=None):
    """(ANY decisions, END decisions) of the pairs (A[i], B[j]) from per-pair oracle calls; A is oligo 1."""
    args = args or oracle.ntthal_args()
    dg = np.empty((len(A), len(B)))
    tt = np.empty((len(A), len(B)))

    def row(i):
        for j, b in enumerate(B):
            r = oracle.thal(tables, A[i], b, oracle.ANY, args)
            dg[i, j] = np.inf if r.no_structure else r.dG
            r = oracle.thal(tables, A[i], b, oracle.END1, args)
            tt[i, j] = 0.0 if r.no_structure else r.t

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(row, range(len(A))))
    return any_rule(oracle, dg, dg_thr), end_rule(oracle, tt, tm_thr)


def enabled(any_cf, end_cf, use_any=True, use_end=True):
    """The two planes with a disabled rule's plane zeroed."""
    z = np.zeros_like(any_cf)
    return (any_cf if use_any else z), (end_cf if use_end else z)


def union(any_cf, end_cf):
    return (any_cf | end_cf).astype(np.uint8)


def block(cf, rows, cols):
    return cf[rows[0]:rows[1], cols[0]:cols[1]]


def row_counts(any_cf, end_cf):
    """Set bits per row of the union: a pair under both rules counts once."""
    return union(any_cf, end_cf).sum(1).astype(np.uint32)


def kind_counts(any_cf, end_cf):
    """[ANY only, END only, both]"""
    a, e = any_cf.astype(bool), end_cf.astype(bool)
    return np.array([(a & ~e).sum(), (e & ~a).sum(), (a & e).sum()], dtype=np.uint64)


def kind_edges(any_cf, end_cf, row0=0, col0=0):
    """Every conflicting pair of the block as (row0 + i, col0 + j, kinds, 0), ascending in (a, b)."""
    kinds = any_cf.astype(np.uint32) * KIND_ANY + end_cf.astype(np.uint32) * KIND_END
    ij = np.argwhere(kinds != 0)                 # row-major: ascending (i, j)
    out = np.zeros(len(ij), dtype=KIND_EDGE)
    out["a"], out["b"] = ij[:, 0] + row0, ij[:, 1] + col0
    out["kinds"] = kinds[ij[:, 0], ij[:, 1]]
    return out


def pack_bits(cf):
    """uint8 (R, C) -> uint64 (R, ceil(C / 64)): bit j % 64 of word j // 64 of row i = cf[i, j], padding clear."""
    R, Cn = cf.shape
    words = (Cn + 63) // 64
    padded = np.zeros((R, words * 64), dtype=np.uint8)
    padded[:, :Cn] = cf != 0
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(R, words)


def unpack_bits(bitmap, ncols):
    return np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8), axis=1, bitorder="little")[:, :ncols]


def by_blocks(any_cf, end_cf, block_rows):
    """The edge list and the row counts put together from row blocks of block_rows, the running count carried from one
    block to the next: what the device does, and equal to the one-piece result whatever block_rows is."""
    parts, counts, base = [], [], 0
    for r0 in range(0, any_cf.shape[0], block_rows):
        a, e = any_cf[r0:r0 + block_rows], end_cf[r0:r0 + block_rows]
        ed = kind_edges(a, e, row0=r0)
        parts.append((base, ed))
        base += len(ed)
        counts.append(row_counts(a, e))
    edges = np.zeros(base, dtype=KIND_EDGE)
    for at, ed in parts:
        edges[at:at + len(ed)] = ed
    return edges, (np.concatenate(counts) if counts else np.zeros(0, np.uint32))
